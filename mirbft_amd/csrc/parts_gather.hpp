// Gathering one action's parts into 64-byte SHA-256 blocks (msha_hash_actions_device,
// parts_kernels.hip k_digest_parts).
//
// ProcessHashActions (pkg/processor/serial.go:180-198) writes an action's Data, a list
// of byte slices, into one hash back to back. Here the slices are (offset, length)
// pairs into an arena; they start at any byte, have any length, may be empty, overlap
// or repeat. One lane walks its action's parts and assembles the byte stream a block
// at a time.
//
// Everything that can go wrong in that -- which source words are read, how they are
// masked by a part's bounds and shifted to the block's byte phase -- is in this
// header, which compiles for the host as well: there a plain array stands in for the
// lane's LDS slot and a callback for the load, and tests/cpp/parts_gather_check.cpp
// runs it under AddressSanitizer against a memcpy concatenation.
//
// The read contract (include/mirsha.h): the only arena reads are whole 16-byte
// granules at multiples of 16 from the arena's base, and a granule is read only when
// it holds at least one byte of a non-empty part.
//
// How a step works. The cursor stands at byte `cur` of a part with `rem` bytes left,
// and the block under assembly holds `pos` bytes. The step takes the
// k = min(16 - cur % 16, rem, 64 - pos) bytes that the granule of `cur` still offers:
//   1. the granule's four dwords are moved down by cur % 16 bytes (whole dwords by
//      two conditional moves, the byte phase by a byte pick from each dword pair),
//      so the k bytes start at byte 0 (bytes past k are whatever followed them);
//   2. they are moved up to the block's byte phase pos % 4 and joined to `acc`, the
//      block's bytes past its last whole dword (kept in a register, never read back);
//   3. the dwords that became whole are written to the slot at pos / 4 ..., and the
//      new partial dword, cut to its valid bytes, is the next `acc`.
// The slot is only ever written in whole dwords at a run-time index (which is why it
// lives in LDS on the GPU: a register array indexed that way would go to scratch);
// no other array here is indexed by a run-time value.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MSHA_HD __host__ __device__ __forceinline__
#else
#define MSHA_HD inline
#endif

namespace msha {
namespace parts {

// One aligned 16-byte granule of the arena as four little-endian dwords.
struct Granule {
  uint32_t d[4];
};

// Bytes [first, first + 4) of the eight bytes lo (0..3), hi (4..7); first in [0, 4].
MSHA_HD uint32_t pick4(uint32_t lo, uint32_t hi, uint32_t first) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(hi, lo, 0x03020100u + first * 0x01010101u);  // v_perm_b32
#else
  return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * first));
#endif
}

// The low nbytes bytes of x (nbytes in [0, 3]).
MSHA_HD uint32_t low_bytes(uint32_t x, uint32_t nbytes) { return x & ~(0xffffffffu << (8 * nbytes)); }

// Where a lane stands in its action's parts. The next part's offset and length are
// fetched one part ahead (noff, nlen), so that a part's first granule can be requested
// as soon as the part before it is used up: the metadata of part j + 1 and the bytes
// of part j are in flight together instead of one after the other.
struct Cursor {
  uint64_t j = 0;     // the part whose offset and length are in noff, nlen (left == 0: none)
  uint32_t left = 0;  // parts not opened yet, part j included (an action has fewer than 2^32)
  uint64_t cur = 0;   // arena offset of the open part's next byte
  uint64_t rem = 0;   // bytes left in the open part (0: none open)
  uint64_t noff = 0, nlen = 0;
};

// The cursor at the start of the n_parts parts from j0. part_off / part_len are read
// only at the action's own indices, here and in fill_block.
MSHA_HD void cursor_init(Cursor& c, uint64_t j0, uint32_t n_parts, const uint64_t* part_off,
                         const uint64_t* part_len) {
  c.j = j0;
  c.left = n_parts;
  c.cur = 0;
  c.rem = 0;
  if (n_parts != 0) {
    c.noff = part_off[j0];
    c.nlen = part_len[j0];
  }
}

// Fills `slot` (16 dwords, written through slot(index, value)) with the next block of
// the stream and returns its byte count: 64 for a whole block, less when the parts ran
// out (then dwords at or past the count's dword are stale or partial: build_tail masks
// them). A whole block leaves nothing pending: blocks end on dword boundaries.
// load(offset) returns the granule at arena + offset, offset a multiple of 16.
template <class SlotWrite, class Load>
MSHA_HD uint32_t fill_block(Cursor& c, const uint64_t* part_off, const uint64_t* part_len, SlotWrite&& slot,
                            Load&& load) {
  uint32_t pos = 0;  // bytes in the block
  uint32_t acc = 0;  // its pos % 4 bytes past the last whole dword, upper bytes zero
  while (pos < 64) {
    while (c.rem == 0 && c.left != 0) {  // open the next part; empty ones contribute nothing
      c.cur = c.noff;
      c.rem = c.nlen;
      ++c.j;
      if (--c.left != 0) {
        c.noff = part_off[c.j];
        c.nlen = part_len[c.j];
      }
    }
    if (c.rem == 0) break;
    const uint32_t lo = (uint32_t)c.cur & 15u;
    uint32_t k = 16u - lo;
    if (k > 64u - pos) k = 64u - pos;
    if (c.rem < k) k = (uint32_t)c.rem;
    const Granule g = load(c.cur - lo);
    c.cur += k;
    c.rem -= k;

    // 1. down by lo bytes: s0..s3 hold the k bytes from byte 0
    uint32_t v0 = g.d[0], v1 = g.d[1], v2 = g.d[2], v3 = g.d[3];
    if (lo & 8u) { v0 = v2; v1 = v3; v2 = 0; v3 = 0; }
    if (lo & 4u) { v0 = v1; v1 = v2; v2 = v3; v3 = 0; }
    const uint32_t sb = lo & 3u;
    const uint32_t s0 = pick4(v0, v1, sb), s1 = pick4(v1, v2, sb), s2 = pick4(v2, v3, sb), s3 = pick4(v3, 0, sb);

    // 2. up to the block's byte phase: o0..o4 are the block's dwords from pos / 4
    const uint32_t db = pos & 3u;
    const uint32_t up = 4u - db;
    const uint32_t o0 = acc | pick4(0, s0, up);
    const uint32_t o1 = pick4(s0, s1, up), o2 = pick4(s1, s2, up), o3 = pick4(s2, s3, up), o4 = pick4(s3, 0, up);

    // 3. whole dwords to the slot, the rest is the new acc
    const uint32_t dd = pos >> 2;
    const uint32_t end = pos + k;
    const uint32_t whole = (end >> 2) - dd;  // 0..4
    if (whole > 0) slot(dd + 0, o0);
    if (whole > 1) slot(dd + 1, o1);
    if (whole > 2) slot(dd + 2, o2);
    if (whole > 3) slot(dd + 3, o3);
    uint32_t part = o0;
    if (whole == 1) part = o1;
    if (whole == 2) part = o2;
    if (whole == 3) part = o3;
    if (whole == 4) part = o4;
    acc = low_bytes(part, end & 3u);
    pos = end;
  }
  if (pos & 3u) slot(pos >> 2, acc);
  return pos;
}

}  // namespace parts
}  // namespace msha
