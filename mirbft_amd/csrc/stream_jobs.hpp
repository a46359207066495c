// Write jobs for the device stream sets (msha_dstreams_write_jobs_device,
// stream_jobs.hip): a flat list of jobs (stream, offset, length) in call order is grouped
// by stream on the GPU, stably, and handed to k_dstream_write as the CSR it wants.
//
// The grouping is a stable LSD radix sort of (key, job index) pairs, key = min(stream,
// n) so that every job naming a stream that is not there sorts behind the valid ones,
// 8 bits a pass. A pass is three kernels -- a digit histogram per tile of kTileJobs
// jobs, an exclusive scan of each digit's row of tile counts (a workgroup a digit, which
// also leaves the digit's total), a stable scatter that starts by scanning the 256
// totals -- and every dependency is a kernel boundary: no workgroup waits on another.
// Inside a tile a job's rank among the jobs of its digit comes from wave ballots (which
// lanes of my wave hold my digit, how many of them are below me), the counts of the
// wave's earlier rounds and the counts of the tile's earlier waves. A position is
//   jobs of lower digits + jobs of that digit in earlier tiles + in earlier waves of the
//   tile + in earlier rounds of the wave + in lower lanes of the round,
// a pure function of the keys: no atomic decides an order.
//
// Everything but the wave intrinsics is in this header, which compiles for the host as
// well (tests/cpp/stream_jobs_check.cpp runs it tile by tile under AddressSanitizer
// against std::stable_sort): the key, the pass count, the digit, where a lane's job
// sits in its tile, the rank from the ballots, the position, the CSR's lower bound and
// the workspace layout.
#pragma once
#include <stdint.h>

#include "parts_gather.hpp"

namespace msha {
namespace sjobs {

constexpr uint32_t kDigitBits = 8;
constexpr uint32_t kDigits = 1u << kDigitBits;
constexpr uint32_t kThreads = 256;  // a workgroup of the histogram and the scatter: a thread a digit
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kRounds = 8;  // jobs a lane ranks, 64 consecutive jobs a round of its wave
constexpr uint32_t kWaveJobs = 64 * kRounds;
constexpr uint32_t kTileJobs = kWaves * kWaveJobs;  // 2,048
constexpr uint32_t kScanThreads = 1024;
constexpr uint32_t kScanPer = 4;  // consecutive counts a thread scans at a time
constexpr uint64_t kMaxJobs = 0xFFFFFFFFull;  // n_jobs stays below it: a job index is 32 bits

static_assert(kThreads == kDigits, "thread t of a tile owns digit t");

// The sort key: the stream, or n for every stream that is not there (n < 2^32 - 1).
MSHA_HD uint32_t clamp_key(uint32_t stream, uint64_t n) { return (uint64_t)stream < n ? stream : (uint32_t)n; }

MSHA_HD uint32_t bit_width(uint64_t x) {
  uint32_t w = 0;
  while (x) {
    ++w;
    x >>= 1;
  }
  return w;
}
// Passes that order keys in [0, n]: 1 up to n = 255, 4 from n = 2^24.
MSHA_HD uint32_t pass_count(uint64_t n) {
  const uint32_t p = (bit_width(n) + kDigitBits - 1) / kDigitBits;
  return p ? p : 1;
}
MSHA_HD uint32_t digit(uint32_t key, uint32_t pass) { return (key >> (kDigitBits * pass)) & (kDigits - 1); }

MSHA_HD uint64_t tile_count(uint64_t n_jobs) { return n_jobs / kTileJobs + (n_jobs % kTileJobs != 0); }
// The counts are digit-major: digit d's row holds its count in every tile, and after the
// scan the digit's jobs in the tiles before. The digits' totals follow the rows.
MSHA_HD uint64_t count_index(uint32_t d, uint64_t tile, uint64_t n_tiles) { return (uint64_t)d * n_tiles + tile; }
MSHA_HD uint64_t total_index(uint32_t d, uint64_t n_tiles) { return (uint64_t)kDigits * n_tiles + d; }
// Where in its tile the job sits that a lane ranks in a round: a wave's rounds are
// consecutive runs of 64 jobs, a tile's waves consecutive runs of rounds.
MSHA_HD uint32_t item_index(uint32_t wave, uint32_t round, uint32_t lane) { return wave * kWaveJobs + round * 64 + lane; }

// The lanes of a round that hold digit d, from the ballot of each digit bit and the
// ballot of the lanes that hold a job at all.
MSHA_HD uint64_t peers(uint32_t d, const uint64_t (&bit_ballot)[kDigitBits], uint64_t valid) {
  uint64_t m = valid;
  for (uint32_t b = 0; b < kDigitBits; ++b) m &= ((d >> b) & 1u) ? bit_ballot[b] : ~bit_ballot[b];
  return m;
}
MSHA_HD uint32_t popcount64(uint64_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popcll(m);
#else
  return (uint32_t)__builtin_popcountll(m);
#endif
}
// Peers in lower lanes: the job's rank inside its round.
MSHA_HD uint32_t lane_rank(uint64_t peer_mask, uint32_t lane) { return popcount64(peer_mask & ((1ull << lane) - 1)); }
// The lowest peer adds the round's count to the wave's.
MSHA_HD bool leads(uint64_t peer_mask, uint32_t lane) { return (peer_mask & ((1ull << lane) - 1)) == 0; }
// lower_digits: the exclusive scan of the digits' totals; earlier_tiles: the (digit,
// tile) entry of the scanned rows; earlier_waves: the digit's jobs in the tile's waves
// before this one; wave_rank: the job's rank among the digit's jobs of its wave (earlier
// rounds, then lower lanes).
MSHA_HD uint64_t scatter_pos(uint32_t lower_digits, uint32_t earlier_tiles, uint32_t earlier_waves,
                             uint32_t wave_rank) {
  return (uint64_t)lower_digits + earlier_tiles + earlier_waves + wave_rank;
}

// The in-tile rank restated serially: jobs before position i of digits[] that hold
// digits[i]. (What peers / lane_rank and the wave and round counts must add up to.)
inline uint32_t serial_rank(const uint32_t* digits, uint32_t i) {
  uint32_t r = 0;
  for (uint32_t j = 0; j < i; ++j) r += digits[j] == digits[i];
  return r;
}

// The first position p in [0, k] with key_at(p) >= t, over keys that do not decrease.
template <class KeyAt>
MSHA_HD uint64_t lower_bound(uint64_t k, uint64_t t, KeyAt&& key_at) {
  uint64_t lo = 0, hi = k;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if ((uint64_t)key_at(mid) < t)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// Which pair buffer a pass writes (0 or 1): they alternate, the first pass reads the
// caller's ids. The sorted pairs are in sorted_buffer().
MSHA_HD uint32_t pass_output(uint32_t pass) { return pass & 1u; }
MSHA_HD uint32_t sorted_buffer(uint32_t passes) { return pass_output(passes - 1); }

// The workspace of a call over k jobs on a set of n streams, byte offsets from a
// 64-byte aligned base: two pair buffers (8 bytes a job each), the grouped offsets and
// lengths (8 each), the tile counts (4 kDigits bytes a tile: half a byte a job) with the
// kDigits totals behind them, and the CSR (8 (n + 1)). ok is false where a size does
// not fit 64 bits.
struct Layout {
  uint64_t pairs[2] = {0, 0}, off = 0, len = 0, counts = 0, begin = 0, bytes = 0;
  uint64_t n_tiles = 0, n_counts = 0;
  bool ok = true;

  Layout(uint64_t k, uint64_t n) {
    n_tiles = tile_count(k);
    n_counts = add(mul(n_tiles, kDigits), kDigits);
    const uint64_t per_job = mul(k, 8);
    pairs[0] = 0;
    pairs[1] = take(per_job);
    off = take(per_job);
    len = take(per_job);
    counts = take(per_job);
    begin = take(mul(n_counts, 4));
    (void)take(mul(add(n, 1), 8));
  }

 private:
  uint64_t mul(uint64_t a, uint64_t b) {
    if (b && a > UINT64_MAX / b) ok = false;
    return ok ? a * b : 0;
  }
  uint64_t add(uint64_t a, uint64_t b) {
    if (a > UINT64_MAX - b) ok = false;
    return ok ? a + b : 0;
  }
  // The running size grows by `size` rounded up to 64; what it was is the next offset.
  uint64_t take(uint64_t size) {
    bytes = add(bytes, add(size, 63) & ~uint64_t(63));
    return bytes;
  }
};

}  // namespace sjobs
}  // namespace msha
