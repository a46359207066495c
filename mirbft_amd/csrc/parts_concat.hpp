// Where the bytes of msha_concat_lists_device go (parts_concat.hip k_concat_copy): a
// list's parts, anywhere in the arena, written back to back into one contiguous,
// 16-byte aligned message.
//
// One workgroup owns a message. It walks the list kStepParts parts at a time: thread t
// holds part t of the step, a block-exclusive scan of the lengths gives every part its
// position in the message, and a running base carries from step to step. The bytes of
// a step reach d_dst through an LDS image of kImageBytes, a window at a time:
//   window   the message bytes [lo, hi), lo where the last one ended, hi at most
//            kImageBytes past wb = lo rounded down to 16: image byte x is message byte
//            wb + x, so a position's phase mod 16 is the same in the image, in the
//            message and (the message starts on a granule) in d_dst;
//   carry    the lo - wb bytes of the granule the window before left incomplete: they
//            are already in the image's first granule;
//   fill     a part shorter than kLargePart is copied by its own thread, a longer one
//            by all threads, a source granule each (copy_piece / coop_piece): the
//            aligned granule is loaded, moved down to byte 0, up to the image's byte
//            phase, and written in whole dwords where all four bytes are the part's
//            and in single bytes at its two ends (put_bytes), so that neighbours
//            sharing a dword never overwrite each other;
//   store    the window's complete granules go to d_dst as whole 16-byte vectors; the
//            (hi - wb) % 16 bytes after them move to the image's start: the carry.
// After the last step the carry, if any, is stored with its pad zeroed (last_granule).
//
// The read contract (include/mirsha.h): the only arena reads are whole 16-byte
// granules at multiples of 16 that hold at least one byte of a non-empty part.
//
// This header compiles for the host as well: tests/cpp/parts_concat_check.cpp replays
// the kernel's loop with it, a plain array for the image and callbacks for the loads
// and stores, under AddressSanitizer + UBSan against a memcpy concatenation.
#pragma once
#include <stdint.h>

#include "parts_gather.hpp"

namespace msha {
namespace parts_concat {

constexpr uint32_t kStepParts = 256;     // S: parts a step takes, one a thread
constexpr uint32_t kLargePart = 512;     // T: parts of T bytes or more are copied by the whole workgroup
constexpr uint32_t kCopyAhead = 4;       // granules a thread loads before it uses the first (copy_piece)
constexpr uint32_t kImageBytes = 16384;  // the LDS image of a window
constexpr uint32_t kScanThreads = 1024;  // k_concat_scan: one workgroup ...
constexpr uint32_t kScanPer = 4;         // ... of this many messages a thread:
constexpr uint32_t kScanWidth = kScanThreads * kScanPer;  // messages an iteration

MSHA_HD uint64_t round16(uint64_t x) { return (x + 15u) & ~uint64_t(15); }

// Does a message of `len` bytes at `off` fit dst_bytes with `slack` bytes after its
// pad? (off + round16(len) + slack <= dst_bytes, without overflow.)
MSHA_HD bool fits(uint64_t off, uint64_t len, uint64_t dst_bytes, uint64_t slack) {
  if (dst_bytes < slack) return false;
  const uint64_t room = dst_bytes - slack;
  if (off > room) return false;
  const uint64_t r = round16(len);
  return r >= len && r <= room - off;
}

// The window that starts at message byte `cur` of a step that ends at `step_end`
// (cur < step_end).
struct Window {
  uint64_t wb;  // message byte of image byte 0: a multiple of 16
  uint64_t lo;  // the window's first new byte; [wb, lo) is the carry
  uint64_t hi;  // one past its last
};
MSHA_HD Window window_at(uint64_t cur, uint64_t step_end) {
  Window w;
  w.wb = cur & ~uint64_t(15);
  w.lo = cur;
  w.hi = step_end < w.wb + kImageBytes ? step_end : w.wb + kImageBytes;
  return w;
}
// Whole granules the window's image holds once filled, and the bytes after them.
MSHA_HD uint32_t window_granules(const Window& w) { return (uint32_t)((w.hi - w.wb) >> 4); }
MSHA_HD uint32_t window_rest(const Window& w) { return (uint32_t)((w.hi - w.wb) & 15u); }

// The piece of a part (message bytes [pos, pos + len)) inside a window: its first
// byte's distance from the part's start, and its length (0: none).
struct Piece {
  uint64_t skip;
  uint64_t n;
};
MSHA_HD Piece clip(uint64_t pos, uint64_t len, const Window& w) {
  const uint64_t a = pos > w.lo ? pos : w.lo;
  const uint64_t e = pos + len;
  const uint64_t b = e < w.hi ? e : w.hi;
  Piece p;
  p.skip = a - pos;
  p.n = b > a ? b - a : 0;
  return p;
}

// The k bytes (1..16 - lo) of granule g from its byte lo, moved down to byte 0 of
// s[0..3] (bytes past k are whatever followed them).
MSHA_HD void shift_down(const parts::Granule& g, uint32_t lo, uint32_t (&s)[4]) {
  uint32_t v0 = g.d[0], v1 = g.d[1], v2 = g.d[2], v3 = g.d[3];
  if (lo & 8u) { v0 = v2; v1 = v3; v2 = 0; v3 = 0; }
  if (lo & 4u) { v0 = v1; v1 = v2; v2 = v3; v3 = 0; }
  const uint32_t sb = lo & 3u;
  s[0] = parts::pick4(v0, v1, sb);
  s[1] = parts::pick4(v1, v2, sb);
  s[2] = parts::pick4(v2, v3, sb);
  s[3] = parts::pick4(v3, 0, sb);
}

// Writes the k bytes (1..16) at byte 0 of s to image bytes [p, p + k): st32(d, v) stores
// image dword d, st8(x, v) image byte x. A dword is stored whole only when all four of
// its bytes are among the k; the others are stored byte by byte.
template <class St32, class St8>
MSHA_HD void put_bytes(uint32_t p, const uint32_t (&s)[4], uint32_t k, St32&& st32, St8&& st8) {
  const uint32_t up = 4u - (p & 3u);  // 1..4: s moved up by p % 4 bytes
  const uint32_t o0 = parts::pick4(0, s[0], up), o1 = parts::pick4(s[0], s[1], up), o2 = parts::pick4(s[1], s[2], up),
                 o3 = parts::pick4(s[2], s[3], up), o4 = parts::pick4(s[3], 0, up);
  const uint32_t d0 = p >> 2, end = p + k;
#define MSHA_CONCAT_PUT(i, o)                                            \
  {                                                                      \
    const uint32_t b0 = 4u * (d0 + (i));                                 \
    if (b0 < end) {                                                      \
      if (b0 >= p && b0 + 4u <= end) {                                   \
        st32(d0 + (i), (o));                                             \
      } else {                                                           \
        if (b0 + 0u >= p && b0 + 0u < end) st8(b0 + 0u, (o) & 0xffu);         \
        if (b0 + 1u >= p && b0 + 1u < end) st8(b0 + 1u, ((o) >> 8) & 0xffu);  \
        if (b0 + 2u >= p && b0 + 2u < end) st8(b0 + 2u, ((o) >> 16) & 0xffu); \
        if (b0 + 3u >= p && b0 + 3u < end) st8(b0 + 3u, ((o) >> 24) & 0xffu); \
      }                                                                  \
    }                                                                    \
  }
  MSHA_CONCAT_PUT(0u, o0)
  MSHA_CONCAT_PUT(1u, o1)
  MSHA_CONCAT_PUT(2u, o2)
  MSHA_CONCAT_PUT(3u, o3)
  MSHA_CONCAT_PUT(4u, o4)
#undef MSHA_CONCAT_PUT
}

// One thread copies arena bytes [src, src + n) to image bytes [p, p + n), a source
// granule after the other. load(offset) returns the granule at arena + offset, offset a
// multiple of 16.
template <class Load, class St32, class St8>
MSHA_HD void copy_piece(uint64_t src, uint64_t n, uint32_t p, Load&& load, St32&& st32, St8&& st8) {
  while (n != 0) {
    // up to kCopyAhead granules a turn, all loads issued before the first is used: a
    // 32-byte part at an odd offset is one round trip to memory instead of three
    const uint32_t lo = (uint32_t)src & 15u;
    const uint64_t g0 = src - lo;
    const uint64_t avail = n + lo;  // the piece ends this many bytes past g0
    parts::Granule g[kCopyAhead];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < kCopyAhead; ++i) {
      g[i] = parts::Granule{{0, 0, 0, 0}};
      if (avail > 16u * i) g[i] = load(g0 + 16u * i);  // granule i holds a byte of the piece
    }
    uint32_t taken = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < kCopyAhead; ++i) {
      if (avail > 16u * i) {
        const uint32_t l = i == 0 ? lo : 0u;
        const uint64_t left = n - taken;
        uint32_t k = 16u - l;
        if (left < k) k = (uint32_t)left;
        uint32_t s[4];
        shift_down(g[i], l, s);
        put_bytes(p + taken, s, k, st32, st8);
        taken += k;
      }
    }
    src += taken;
    p += taken;
    n -= taken;
  }
}

// The same piece copied by `threads` threads: thread t takes the source granules t,
// t + threads, ... of those the piece touches, one load each.
template <class Load, class St32, class St8>
MSHA_HD void coop_piece(uint64_t src, uint64_t n, uint32_t p, uint32_t t, uint32_t threads, Load&& load, St32&& st32,
                        St8&& st8) {
  if (n == 0) return;
  const uint64_t g0 = src >> 4, ng = ((src + n + 15u) >> 4) - g0;
  for (uint64_t i = t; i < ng; i += threads) {
    const uint64_t gb = (g0 + i) << 4;
    const uint64_t a = gb > src ? gb : src;
    const uint64_t b = gb + 16u < src + n ? gb + 16u : src + n;
    const parts::Granule g = load(gb);
    uint32_t s[4];
    shift_down(g, (uint32_t)(a - gb), s);
    put_bytes(p + (uint32_t)(a - src), s, (uint32_t)(b - a), st32, st8);
  }
}

// The message's last granule when its length is no multiple of 16: the r = len % 16
// carried bytes (image dwords v[0..3]) with the pad zeroed.
MSHA_HD void last_granule(uint32_t (&v)[4], uint32_t r) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t j = 0; j < 4; ++j) {
    const uint32_t have = r > 4u * j ? r - 4u * j : 0u;  // bytes of dword j that are the message's
    v[j] = have >= 4u ? v[j] : parts::low_bytes(v[j], have);
  }
}

}  // namespace parts_concat
}  // namespace msha
