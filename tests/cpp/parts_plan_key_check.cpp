// The block-count -> class-key function of msha_hash_actions_device_planned
// (mirbft_amd/csrc/parts_plan.hpp) as a stand-alone host program, built with
// -fsanitize=address,undefined by tests/test_parts_plan_abi.py. For every block count
// on the command line (decimal) it prints "blocks key", after checking the key against
// a restatement written without the header's helpers (a linear search for the class)
// and the properties the planner relies on: keys below kKeys, non-increasing in the
// block count, exact classes below 4,096 blocks. It also walks every length 0..8191
// through blocks_for_len against the padding rule spelled out.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../mirbft_amd/csrc/parts_plan.hpp"

namespace pp = msha::parts_plan;

static uint32_t key_restated(uint64_t blocks) {
  if (blocks < 4096) return 52 + 4095 - (uint32_t)blocks;
  // classes [2^e, 2^(e+1)), e = 12..63; the longest class has key 0
  for (uint32_t e = 63; e >= 12; --e)
    if (blocks >> e) return 63 - e;
  return ~0u;
}

int main(int argc, char** argv) {
  std::vector<uint64_t> blocks;
  for (int i = 1; i < argc; ++i) blocks.push_back(std::strtoull(argv[i], nullptr, 10));
  int bad = 0;
  for (uint64_t b : blocks) {
    const uint32_t k = pp::class_key(b);
    if (k != key_restated(b) || k >= pp::kKeys) {
      std::printf("MISMATCH blocks %" PRIu64 ": key %u, restated %u\n", b, k, key_restated(b));
      ++bad;
    }
    if (b > 0 && pp::class_key(b - 1) < k) {
      std::printf("NOT MONOTONE at blocks %" PRIu64 "\n", b);
      ++bad;
    }
    if (b > 0 && b < 4096 && pp::class_key(b - 1) != k + 1) {
      std::printf("NOT EXACT at blocks %" PRIu64 "\n", b);
      ++bad;
    }
    std::printf("%" PRIu64 " %u\n", b, k);
  }
  for (uint64_t len = 0; len < 8192; ++len) {
    const uint64_t want = len / 64 + 1 + (len % 64 >= 56 ? 1 : 0);  // 0x80 and the 8-byte length must fit
    if (pp::blocks_for_len(len) != want) {
      std::printf("BLOCKS MISMATCH len %" PRIu64 "\n", len);
      ++bad;
    }
  }
  if (pp::class_key(0) != pp::kKeys - 1 || pp::class_key(~0ull) != 0) {
    std::printf("KEY RANGE: key(0) %u, key(max) %u\n", pp::class_key(0), pp::class_key(~0ull));
    ++bad;
  }
  if (bad) return 1;
  std::printf("parts_plan keys ok: %zu block counts\n", blocks.size());
  return 0;
}
