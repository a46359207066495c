// The lane order of msha_hash_actions_device_planned (parts_plan.hip): from a list's
// byte total to its SHA-256 block count to its block-count class. Lanes run in
// descending class order, so a wave of k_digest_parts_planned holds lists of (nearly)
// one block count and no lane waits long for its wave's longest.
//
// The classes are the existing planner's (kernels.hpp FoldArgs): the exact block count
// below 4,096 blocks, powers of two from there up. Keys are descending classes -- key 0
// is the longest class -- so bucket starts are a plain prefix sum over the keys.
//
// This header compiles for the host as well: tests/cpp/parts_plan_key_check.cpp runs
// it under AddressSanitizer + UBSan against a restatement, and
// tests/cpp/call_workspace_check.cpp the workspace layout.
#pragma once
#include <stdint.h>

#include "workspace_rule.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MSHA_PLAN_HD __host__ __device__ __forceinline__
#else
#define MSHA_PLAN_HD inline
#endif

namespace msha {
namespace parts_plan {

constexpr uint32_t kExactBlocks = 4096;                     // block counts below this are classes of their own
constexpr uint32_t kBigClasses = 52;                        // 2^12 .. 2^63: keys [0, 52)
constexpr uint32_t kKeys = kBigClasses + kExactBlocks;      // 4,148; block count 0 has the last key
constexpr uint16_t kNoKey = 0xFFFF;                         // a list no action names

// Lists of at least this many parts are summed by their whole wave (coalesced part_len
// loads and a wave reduction), shorter ones by their own lane. Chosen by measurement:
// profiles/parts_planned/README.md. MSHA_PARTS_PLAN_WAVE_SUM overrides it for A/B runs.
constexpr uint32_t kWaveSumParts = 32;

// 64-byte compressions of an L-byte message (FIPS 180-4 5.1.1; msha_blocks_for_len).
MSHA_PLAN_HD uint64_t blocks_for_len(uint64_t len) { return (len >> 6) + ((len & 63) < 56 ? 1 : 2); }

// floor(log2(x)) for x >= 1.
MSHA_PLAN_HD uint32_t log2_floor(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return 63u - (uint32_t)__clzll((long long)x);
#else
  return 63u - (uint32_t)__builtin_clzll(x);
#endif
}

// The key of a list of `blocks` blocks: non-increasing in blocks, below kKeys.
MSHA_PLAN_HD uint32_t class_key(uint64_t blocks) {
  if (blocks >= kExactBlocks) return 63u - log2_floor(blocks);
  return kBigClasses + (kExactBlocks - 1u) - (uint32_t)blocks;
}

// The workspace of a call over n lists (n < 2^32), byte offsets from its base: info (16
// words) and the counters, one array to k_parts_init, lie at 0; then the order, at an
// offset that does not depend on n (msha_parts_plan_read_order reads it after the call);
// then the keys, the used flags and the digest table. at: where the order lies -- behind
// the counters, or behind what another entry puts between them (parts_route.hpp Layout).
MSHA_HD uint64_t head_bytes() { return round64(4ull * (16 + kKeys)); }
struct Layout {
  uint64_t order, key16, used, table, bytes;
  MSHA_HD Layout(uint64_t n, bool with_list, uint64_t at = head_bytes()) {
    order = at;
    key16 = order + round64(4 * n);
    used = key16 + round64(2 * n);
    table = used + (with_list ? round64(n) : 0);
    bytes = table + (with_list ? 32 * n : 0) + 64;
  }
};

}  // namespace parts_plan
}  // namespace msha
