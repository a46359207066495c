// How msha_verify_digests_device (include/mirsha.h "Digests verified on the GPU";
// verify.hip) lays out its answer and walks it.
//
//   mask   slot i is bit bit_of(i) of word word_of(i); a call writes all mask_words(n)
//          words, and valid_bits() says which bits of a word are slots at all (the bits at
//          and past n in the last word are 0).
//   match  differs(): slot i against expected row e = idx ? idx[i] : i, the OR of the XOR
//          of the eight dwords, each side two 16-byte granules; e >= n_expected differs
//          and no granule of d_expected is loaded.
//   walk   k_verify_scan is ONE workgroup of kScanThreads threads. It walks the mask
//          kScanWords words a chunk, thread t holding word w0 + t: a popcount per thread,
//          a workgroup-exclusive prefix of them (the `prefix` callback: wave shuffles and
//          LDS on the GPU), and a running base carried from chunk to chunk, so that the
//          k-th set bit of the whole mask has rank k. emit_word() then writes the slots of
//          a word's set bits at their ranks, in bit order, while the rank is below
//          list_cap; nothing is written at or past min(bad, list_cap). The same pass
//          keeps, per thread, the smallest set slot and how many set slots have an
//          expected index out of range (d_expected_idx is read again for set bits only:
//          the call has no workspace for a second mask, and nothing else needs one).
//
// This header compiles for the host as well: tests/cpp/verify_check.cpp runs compare and
// walk with it under AddressSanitizer + UBSan, every array at exactly its contract size.
#pragma once
#include <stdint.h>

#include "parts_gather.hpp"

namespace msha {
namespace verify {

constexpr uint32_t kCompareThreads = 256;    // k_verify_compare: a lane a slot, four mask words a workgroup
constexpr uint32_t kScanThreads = 1024;      // k_verify_scan: one workgroup ...
constexpr uint32_t kScanWords = kScanThreads;  // ... of one mask word a thread and chunk (msha_verify_stats.scan_words)

MSHA_HD uint64_t word_of(uint64_t slot) { return slot >> 6; }
MSHA_HD uint32_t bit_of(uint64_t slot) { return (uint32_t)(slot & 63u); }
MSHA_HD uint64_t mask_words(uint64_t n) { return (n + 63u) >> 6; }
// The bits of mask word w that are slots below n (w < mask_words(n): never 0).
MSHA_HD uint64_t valid_bits(uint64_t w, uint64_t n) {
  const uint64_t first = w << 6;
  if (first >= n) return 0;
  const uint64_t left = n - first;
  return left >= 64u ? ~uint64_t(0) : (uint64_t(1) << left) - 1u;
}

// Does slot i differ from its expected row? idx(i): d_expected_idx[i], called only with
// has_idx; got(i, h) / exp(e, h): half h (0, 1) of a 32-byte row as a granule. exp is
// not called for e >= n_expected.
template <class Idx, class Got, class Exp>
MSHA_HD bool differs(uint64_t i, uint64_t n_expected, bool has_idx, Idx&& idx, Got&& got, Exp&& exp) {
  const uint64_t e = has_idx ? (uint64_t)idx(i) : i;
  if (e >= n_expected) return true;
  const parts::Granule g0 = got(i, 0u), g1 = got(i, 1u);
  const parts::Granule x0 = exp(e, 0u), x1 = exp(e, 1u);
  uint32_t acc = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t k = 0; k < 4; ++k) acc |= (g0.d[k] ^ x0.d[k]) | (g1.d[k] ^ x1.d[k]);
  return acc != 0;
}

// What a thread of the walk carries: the smallest set slot it saw (kNone: none) and its
// set slots whose expected index is out of range.
constexpr uint64_t kNone = ~uint64_t(0);
struct Seen {
  uint64_t first = kNone;
  uint64_t bad_index = 0;
};

// The set bits of mask word w (value m), whose first has rank `rank`: put(r, slot) for
// each, in bit order, while r < list_cap; bad_idx(slot) (asked only with has_idx) says
// whether the slot's expected index is out of range.
template <class Put, class BadIdx>
MSHA_HD void emit_word(uint64_t w, uint64_t m, uint64_t rank, uint64_t list_cap, bool has_idx, Put&& put,
                       BadIdx&& bad_idx, Seen* seen) {
  if (m == 0) return;
  const uint64_t lowest = (w << 6) + (uint64_t)__builtin_ctzll(m);
  if (lowest < seen->first) seen->first = lowest;
  if (!has_idx && rank >= list_cap) return;  // nothing left to write or to count
  while (m != 0) {
    const uint64_t slot = (w << 6) + (uint64_t)__builtin_ctzll(m);
    m &= m - 1u;
    if (rank < list_cap) put(rank, (uint32_t)slot);
    if (has_idx && bad_idx(slot)) seen->bad_index++;
    ++rank;
  }
}

// Thread t's part of the walk over `words` mask words. load(w): mask word w;
// prefix(count, &before, &all): the sum of `count` over the threads below t and over
// all threads of this chunk (every thread calls it once a chunk, so it may hold
// barriers). Returns the number of set bits of the whole mask.
template <class Load, class Prefix, class Put, class BadIdx>
MSHA_HD uint64_t walk(uint64_t words, uint32_t t, uint64_t list_cap, bool has_idx, Load&& load, Prefix&& prefix,
                      Put&& put, BadIdx&& bad_idx, Seen* seen) {
  uint64_t base = 0;
  for (uint64_t w0 = 0; w0 < words; w0 += kScanWords) {
    const uint64_t w = w0 + t;
    const uint64_t m = w < words ? load(w) : 0;
    uint32_t before = 0, all = 0;
    prefix((uint32_t)__builtin_popcountll(m), &before, &all);
    emit_word(w, m, base + before, list_cap, has_idx, put, bad_idx, seen);
    base += all;
  }
  return base;
}

// msha_verify_result's five words, in its field order.
MSHA_HD void result_words(uint64_t n, uint64_t bad, uint64_t first, uint64_t list_cap, uint64_t bad_index,
                          uint64_t (&r)[5]) {
  r[0] = n;
  r[1] = bad;
  r[2] = bad == 0 ? n : first;
  r[3] = bad < list_cap ? bad : list_cap;
  r[4] = bad_index;
}

}  // namespace verify
}  // namespace msha
