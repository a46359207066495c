// msha_verify_digests_device (gfx950 only): digests compared with the ones the caller
// expects, the answer left in HBM (include/mirsha.h "Digests verified on the GPU").
//
// Two kernels on the caller's stream, no workspace, no memset, no host wait:
//   k_verify_compare  a lane a slot: both rows as two 16-byte loads each, the OR of the
//                     XOR of the eight dwords, a wave ballot of "differs", and lane 0 of
//                     the wave stores the 64-bit mask word (a wave is a word). Lanes at
//                     and past n contribute 0; the grid covers whole words, so every
//                     word of the mask is written. An expected index out of range
//                     differs and loads nothing of d_expected.
//   k_verify_scan     ONE workgroup walks the mask verify::kScanWords words a chunk with
//                     a carry (verify.hpp walk): ranks -> d_bad_list, then the counts,
//                     the first differing slot and the out-of-range count -> d_result.
//                     Nothing waits for another workgroup, so nothing can spin, and no
//                     word that nobody zeroed is added to.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mirsha.h"
#include "kernels.hpp"
#include "verify.hpp"

namespace msha {

namespace {

namespace vf = verify;

__device__ __forceinline__ uint32_t wave_lane() { return threadIdx.x & 63u; }

// Inclusive scan over the wave.
__device__ __forceinline__ uint32_t wave_scan(uint32_t v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(v, d);
    if ((int)wave_lane() >= d) v += up;
  }
  return v;
}

__device__ __forceinline__ parts::Granule load_granule(const uint8_t* p) {
  const uint4 v = *reinterpret_cast<const uint4*>(p);
  parts::Granule g;
  g.d[0] = v.x;
  g.d[1] = v.y;
  g.d[2] = v.z;
  g.d[3] = v.w;
  return g;
}

__global__ __launch_bounds__(vf::kCompareThreads) void k_verify_compare(VerifyArgs a) {
  static_assert(vf::kCompareThreads % 64 == 0, "a wave is one mask word");
  const uint64_t i = (uint64_t)blockIdx.x * vf::kCompareThreads + threadIdx.x;
  bool d = false;
  if (i < a.n)
    d = vf::differs(
        i, a.n_expected, a.expected_idx != nullptr, [&](uint64_t s) { return a.expected_idx[s]; },
        [&](uint64_t s, uint32_t h) { return load_granule(a.got + 32u * s + 16u * h); },
        [&](uint64_t e, uint32_t h) { return load_granule(a.expected + 32u * e + 16u * h); });
  const uint64_t m = __ballot(d);
  const uint64_t w = vf::word_of(i);  // the same for the whole wave
  if (wave_lane() == 0 && w < vf::mask_words(a.n)) a.bad_mask[w] = m & vf::valid_bits(w, a.n);
}

__global__ __launch_bounds__(vf::kScanThreads) void k_verify_scan(VerifyArgs a) {
  constexpr uint32_t kWaves = vf::kScanThreads / 64;
  __shared__ uint32_t wsum[kWaves];
  __shared__ uint64_t s_first[kWaves], s_bad_index[kWaves];
  const uint32_t t = threadIdx.x;
  const bool has_idx = a.expected_idx != nullptr;

  auto prefix = [&](uint32_t c, uint32_t* before, uint32_t* all) {
    const uint32_t inc = wave_scan(c);
    if (wave_lane() == 63) wsum[t >> 6] = inc;
    __syncthreads();
    uint32_t b = 0, s = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) {
      if (w < (t >> 6)) b += wsum[w];
      s += wsum[w];
    }
    *before = b + inc - c;
    *all = s;
    __syncthreads();  // wsum is written again
  };

  vf::Seen seen;
  const uint64_t bad = vf::walk(
      vf::mask_words(a.n), t, a.list_cap, has_idx, [&](uint64_t w) { return a.bad_mask[w]; }, prefix,
      [&](uint64_t r, uint32_t slot) { a.bad_list[r] = slot; },
      [&](uint64_t slot) { return (uint64_t)a.expected_idx[slot] >= a.n_expected; }, &seen);

  uint64_t first = seen.first, bad_index = seen.bad_index;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint64_t of = __shfl_xor((unsigned long long)first, d);
    first = of < first ? of : first;
    bad_index += __shfl_xor((unsigned long long)bad_index, d);
  }
  if (wave_lane() == 0) {
    s_first[t >> 6] = first;
    s_bad_index[t >> 6] = bad_index;
  }
  __syncthreads();
  if (t == 0) {
    first = vf::kNone;
    bad_index = 0;
    for (uint32_t w = 0; w < kWaves; ++w) {
      first = s_first[w] < first ? s_first[w] : first;
      bad_index += s_bad_index[w];
    }
    uint64_t r[5];
    vf::result_words(a.n, bad, first, a.list_cap, bad_index, r);
#pragma unroll
    for (uint32_t k = 0; k < 5; ++k) a.result[k] = r[k];
  }
}

}  // namespace

hipError_t launch_verify_compare(const VerifyArgs& a, hipStream_t st) {
  // n < 2^32 - 1 (the host's bound): at most 2^24 workgroups
  const unsigned grid = (unsigned)((a.n + vf::kCompareThreads - 1) / vf::kCompareThreads);
  hipLaunchKernelGGL(k_verify_compare, dim3(grid), dim3(vf::kCompareThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_verify_scan(const VerifyArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_verify_scan, dim3(1), dim3(vf::kScanThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace msha
