// msha_hash_actions_device_planned (gfx950 only): multi-part actions named through
// part LISTS, planned and folded on the GPU inside the call.
//
// Actions name lists (action_list[i], or action i = list i), lists own parts. A list
// named by many actions is hashed once -- aliasing is an integer compare, no content is
// hashed or compared for it -- and a list nobody names is never touched. The named
// lists are the lanes of k_digest_parts_planned, in descending block-count class
// (parts_plan.hpp), so a wave's lanes finish together.
//
// Seven kernels on the caller's stream, no host round trip between them (and no
// memset: the workspace is reset by a kernel, so a captured call is kernel nodes only):
//   k_parts_init     zeroes the counters (and the used flags), fills `order` with kNoLane
//   k_parts_mark     (with action_list) used[list] = 1 per action; an id >= n_lists
//                    raises kErrPartsList
//   k_parts_measure  per used list: bytes = sum of its part lengths -> blocks -> class
//                    key (key16), a histogram of the keys (cnt) and the block sum
//   k_parts_scan     one workgroup: cnt -> bucket starts by ascending key (descending
//                    class), info[0] = lanes
//   k_parts_scatter  list -> its position in `order` (positions past the lane count
//                    keep kNoLane)
//   k_digest_parts_planned  k_digest_parts' lane (parts_digest.hpp) over `order`
//   k_parts_fill     (with action_list) out[i] = table[action_list[i]], zeros for an id
//                    out of range
//
// Summing a list's lengths. A lane sums a short list itself. A list of T parts or more
// (PartsPlanArgs::wave_sum_parts, parts_plan.hpp kWaveSumParts) is summed by its whole
// wave, one such list after the other: 64 consecutive part_len words a load, a
// butterfly reduction, the total handed back to the list's lane. An EpochChange list
// has some 2,000 parts: 32 coalesced loads a lane instead of 2,000 one after the other.
//
// The histogram is kept in LDS per workgroup (4,148 counters, 16.6 KB) and added to
// the global counters once per key the workgroup saw. A wave whose lanes all hold one
// key (uniform batches; most waves of a sorted or clustered one) adds its population
// count with one LDS atomic instead of 64 on one address (hist_add).
//
// msha_hash_actions_device_routed runs the same sequence with two kernels of its own in
// place of the first and the third (launch_parts_route_plan): k_route_init also resets
// the route's slots, and k_route_measure, which has the lengths in hand, decides which
// lists leave the lanes for the eight-lane chain (parts_route.hpp). The host then puts
// k_concat_copy and the chain launch between the scatter and k_digest_parts_planned.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "parts_digest.hpp"
#include "parts_plan.hpp"
#include "parts_route.hpp"

namespace msha {

namespace {

using parts_plan::kKeys;
using parts_plan::kNoKey;

__device__ __forceinline__ uint32_t wave_lane() { return threadIdx.x & 63u; }

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor((unsigned long long)v, d);
  return v;
}

// h[key] += 1 for every lane with `valid`; returns what h[key] held before this lane's
// increment (lanes of one key get consecutive values). Every lane of the wave calls it.
__device__ __forceinline__ uint32_t hist_add(uint32_t* h, uint32_t key, bool valid) {
  const uint64_t m = __ballot(valid);
  if (m == 0) return 0;
  const int lead = __ffsll((unsigned long long)m) - 1;
  const uint32_t k0 = (uint32_t)__shfl((int)key, lead);
  if (__ballot(valid && key != k0) == 0) {  // one key in the wave: one atomic
    uint32_t base = 0;
    if ((int)wave_lane() == lead) base = atomicAdd(&h[k0], (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, lead);
    return base + (uint32_t)__popcll(m & ((1ull << wave_lane()) - 1ull));
  }
  return valid ? atomicAdd(&h[key], 1u) : 0u;
}

// info and cnt are one array of 16 + kKeys words; used is rounded up to whole words.
__global__ __launch_bounds__(256) void k_parts_init(PartsPlanArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 16 + kKeys) a.info[i] = 0;
  if (i < a.n_lists) a.order[i] = kNoLane;
  if (a.used && i < (a.n_lists + 3) / 4) reinterpret_cast<uint32_t*>(a.used)[i] = 0;
}

__global__ __launch_bounds__(256) void k_parts_mark(PartsPlanArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_actions) return;
  const uint32_t l = a.action_list[i];
  if (l < a.n_lists) {
    a.used[l] = 1;  // every writer stores the same byte
  } else {
    atomicOr(a.err, kErrPartsList);
  }
}

__global__ __launch_bounds__(256) void k_parts_measure(PartsPlanArgs a) {
  __shared__ uint32_t hist[kKeys];
  __shared__ unsigned long long bsum;
  for (uint32_t k = threadIdx.x; k < kKeys; k += blockDim.x) hist[k] = 0;
  if (threadIdx.x == 0) bsum = 0;
  __syncthreads();

  const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool lane = l < a.n_lists && (!a.used || a.used[l] != 0);
  uint64_t j0 = 0, np = 0;
  bool bad = false;
  if (lane) {
    j0 = a.begin[l];
    const uint64_t jend = a.begin[l + 1];
    // the hash lane flags and zeroes such a list (parts_digest.hpp); here it is a lane of no blocks
    bad = jend < j0 || jend - j0 > 0xffffffffull;
    np = bad ? 0 : jend - j0;
  }
  const bool wide = lane && np >= a.wave_sum_parts;
  uint64_t total = 0;
  if (lane && !wide)
    for (uint64_t j = 0; j < np; ++j) total += a.part_len[j0 + j];
  // the long lists of this wave, one after the other, by all 64 lanes (only list
  // indices of lists in use are read: [wj0, wj0 + wnp))
  uint64_t pending = __ballot(wide);
  while (pending) {
    const int lead = __ffsll((unsigned long long)pending) - 1;
    pending &= pending - 1;
    const uint64_t wj0 = __shfl((unsigned long long)j0, lead), wnp = __shfl((unsigned long long)np, lead);
    uint64_t s = 0;
    for (uint64_t j = wave_lane(); j < wnp; j += 64) s += a.part_len[wj0 + j];
    s = wave_sum(s);
    if ((int)wave_lane() == lead) total = s;
  }
  const uint64_t blocks = (lane && !bad) ? parts_plan::blocks_for_len(total) : 0;
  const uint32_t key = lane ? parts_plan::class_key(blocks) : kNoKey;
  if (l < a.n_lists) a.key16[l] = (uint16_t)key;
  (void)hist_add(hist, key, lane);
  const uint64_t wblocks = wave_sum(blocks);
  if (wave_lane() == 0 && wblocks) atomicAdd(&bsum, (unsigned long long)wblocks);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < kKeys; k += blockDim.x) {
    const uint32_t c = hist[k];
    if (c) atomicAdd(&a.cnt[k], c);
  }
  if (threadIdx.x == 0 && bsum) atomicAdd(reinterpret_cast<unsigned long long*>(a.info + 2), bsum);
}

// cnt[k] (lanes of key k) -> the first position of key k, keys ascending; info[0] = lanes.
constexpr uint32_t kScanThreads = 1024;
constexpr uint32_t kScanPer = (kKeys + kScanThreads - 1) / kScanThreads;
__global__ __launch_bounds__(kScanThreads) void k_parts_scan(PartsPlanArgs a) {
  __shared__ uint32_t wsum[kScanThreads / 64];
  const uint32_t k0 = threadIdx.x * kScanPer;
  uint32_t c[kScanPer], s = 0;
#pragma unroll
  for (uint32_t j = 0; j < kScanPer; ++j) {
    c[j] = k0 + j < kKeys ? a.cnt[k0 + j] : 0;
    s += c[j];
  }
  uint32_t inc = s;  // inclusive scan over the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)inc, d);
    if ((int)wave_lane() >= d) inc += up;
  }
  if (wave_lane() == 63) wsum[threadIdx.x >> 6] = inc;
  __syncthreads();
  uint32_t base = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < kScanThreads / 64; ++w) {
    if (w < (threadIdx.x >> 6)) base += wsum[w];
    all += wsum[w];
  }
  uint32_t start = base + inc - s;
#pragma unroll
  for (uint32_t j = 0; j < kScanPer; ++j) {
    if (k0 + j < kKeys) a.cnt[k0 + j] = start;
    start += c[j];
  }
  if (threadIdx.x == 0) a.info[0] = all;
}

__global__ __launch_bounds__(256) void k_parts_scatter(PartsPlanArgs a) {
  __shared__ uint32_t hist[kKeys];
  for (uint32_t k = threadIdx.x; k < kKeys; k += blockDim.x) hist[k] = 0;
  __syncthreads();
  const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t key = l < a.n_lists ? a.key16[l] : kNoKey;
  const bool lane = key < kKeys;
  (void)hist_add(hist, key, lane);
  __syncthreads();
  // the workgroup's share of each bucket it has lanes in: count -> first position
  for (uint32_t k = threadIdx.x; k < kKeys; k += blockDim.x) {
    const uint32_t c = hist[k];
    if (c) hist[k] = atomicAdd(&a.cnt[k], c);
  }
  __syncthreads();
  const uint32_t pos = hist_add(hist, key, lane);
  if (lane && pos < a.n_lists) a.order[pos] = (uint32_t)l;
}

__global__ __launch_bounds__(256, 8) void k_digest_parts_planned(const uint8_t* __restrict__ arena,
                                                                const uint64_t* __restrict__ part_off,
                                                                const uint64_t* __restrict__ part_len,
                                                                const uint64_t* __restrict__ begin,
                                                                const uint32_t* __restrict__ order, uint64_t n,
                                                                uint8_t* __restrict__ out, uint32_t* __restrict__ err) {
  __shared__ uint32_t slots[256 * kPartsSlotStride];
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t a = order[i];
  if (a == kNoLane) return;  // past the lane count: lists nobody names
  digest_parts_lane(arena, part_off, part_len, begin, (uint64_t)a, out, err, slots);
}

__global__ __launch_bounds__(256) void k_parts_fill(PartsPlanArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_actions) return;
  const uint32_t l = a.action_list[i];
  uint4 x0 = make_uint4(0, 0, 0, 0), x1 = x0;
  if (l < a.n_lists) {
    const uint4* src = reinterpret_cast<const uint4*>(a.table + 32 * (uint64_t)l);
    x0 = src[0];  // both loads before either store
    x1 = src[1];
  }
  uint4* dst = reinterpret_cast<uint4*>(a.out + 32 * i);
  dst[0] = x0;
  dst[1] = x1;
}

// msha_hash_actions_device_routed: k_parts_init's reset plus the route's arrays -- every
// slot back to unfilled, the claim counters to 0 -- so a call leaves nothing for the next.
__global__ __launch_bounds__(256) void k_route_init(PartsPlanArgs a, RouteArgs r) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 16 + kKeys) a.info[i] = 0;
  if (i < a.n_lists) a.order[i] = kNoLane;
  if (a.used && i < (a.n_lists + 3) / 4) reinterpret_cast<uint32_t*>(a.used)[i] = 0;
  if (i < r.max_long) {
    r.sel[i] = 0;
    r.msg_off[i] = 0;
    r.msg_len[i] = parts_route::kUnfilledLen;
    r.chain_order[i] = parts_route::kUnfilledOrder;
    r.out_idx[i] = 0;
  }
  if (i < parts_route::kClaimWords) r.claim[i] = 0;
}

// k_parts_measure with the routing decision: a valid list of long_blocks blocks or more
// claims a slot and room (parts_route.hpp). With both it is the chain's -- its slot
// filled, its key kNoKey, out of the histogram and the block sum -- and otherwise it is
// a lane as every other list is. The claim is settled before hist_add, whose `valid` is
// per lane while its one-atomic path is per wave: a list counts there once or not at all.
__global__ __launch_bounds__(256) void k_route_measure(PartsPlanArgs a, RouteArgs r) {
  __shared__ uint32_t hist[kKeys];
  __shared__ unsigned long long bsum;
  for (uint32_t k = threadIdx.x; k < kKeys; k += blockDim.x) hist[k] = 0;
  if (threadIdx.x == 0) bsum = 0;
  __syncthreads();

  const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool named = l < a.n_lists && (!a.used || a.used[l] != 0);
  uint64_t j0 = 0, np = 0;
  bool bad = false;
  if (named) {
    j0 = a.begin[l];
    const uint64_t jend = a.begin[l + 1];
    bad = jend < j0 || jend - j0 > 0xffffffffull;
    np = bad ? 0 : jend - j0;
  }
  const bool wide = named && np >= a.wave_sum_parts;
  uint64_t total = 0;
  if (named && !wide)
    for (uint64_t j = 0; j < np; ++j) total += a.part_len[j0 + j];
  uint64_t pending = __ballot(wide);
  while (pending) {
    const int lead = __ffsll((unsigned long long)pending) - 1;
    pending &= pending - 1;
    const uint64_t wj0 = __shfl((unsigned long long)j0, lead), wnp = __shfl((unsigned long long)np, lead);
    uint64_t s = 0;
    for (uint64_t j = wave_lane(); j < wnp; j += 64) s += a.part_len[wj0 + j];
    s = wave_sum(s);
    if ((int)wave_lane() == lead) total = s;
  }
  uint64_t blocks = (named && !bad) ? parts_plan::blocks_for_len(total) : 0;

  bool routed = false;
  uint64_t next = 0;
  if (named && !bad && parts_route::is_long(blocks, r.long_blocks) &&
      parts_route::room_ok(0, total, r.long_bytes, kArenaSlack, &next)) {  // (could it ever fit?)
    const uint64_t ticket = atomicAdd(&r.claim[parts_route::kClaimSlots], 1ull);
    if (parts_route::slot_ok(ticket, r.max_long)) {
      unsigned long long* const given = &r.claim[parts_route::kClaimBytes];
      uint64_t cur = __atomic_load_n(given, __ATOMIC_RELAXED);
      while (parts_route::room_ok(cur, total, r.long_bytes, kArenaSlack, &next)) {
        const uint64_t seen = atomicCAS(given, (unsigned long long)cur, (unsigned long long)next);
        if (seen == cur) {
          routed = true;
          break;
        }
        cur = seen;
      }
      if (routed) {
        const uint32_t s = (uint32_t)ticket;
        r.sel[s] = (uint32_t)l;
        r.msg_off[s] = cur;
        r.msg_len[s] = total;
        r.chain_order[s] = s;
        r.out_idx[s] = (uint32_t)l;
        atomicAdd(&r.claim[parts_route::kClaimRouted], 1ull);
      }
    }
  }
  const bool lane = named && !routed;
  if (routed) blocks = 0;
  const uint32_t key = lane ? parts_plan::class_key(blocks) : kNoKey;
  if (l < a.n_lists) a.key16[l] = (uint16_t)key;
  (void)hist_add(hist, key, lane);
  const uint64_t wblocks = wave_sum(blocks);
  if (wave_lane() == 0 && wblocks) atomicAdd(&bsum, (unsigned long long)wblocks);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < kKeys; k += blockDim.x) {
    const uint32_t c = hist[k];
    if (c) atomicAdd(&a.cnt[k], c);
  }
  if (threadIdx.x == 0 && bsum) atomicAdd(reinterpret_cast<unsigned long long*>(a.info + 2), bsum);
}

unsigned grid256(uint64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

hipError_t launch_parts_route_plan(const PartsPlanArgs& a, const RouteArgs& r, hipStream_t st, uint32_t* launches) {
  uint32_t k = 1;
  uint64_t words = a.n_lists > 16 + kKeys ? a.n_lists : 16 + kKeys;
  if (r.max_long > words) words = r.max_long;
  hipLaunchKernelGGL(k_route_init, dim3(grid256(words)), dim3(256), 0, st, a, r);
  if (a.action_list) {
    hipLaunchKernelGGL(k_parts_mark, dim3(grid256(a.n_actions)), dim3(256), 0, st, a);
    ++k;
  }
  hipLaunchKernelGGL(k_route_measure, dim3(grid256(a.n_lists)), dim3(256), 0, st, a, r);
  hipLaunchKernelGGL(k_parts_scan, dim3(1), dim3(kScanThreads), 0, st, a);
  hipLaunchKernelGGL(k_parts_scatter, dim3(grid256(a.n_lists)), dim3(256), 0, st, a);
  if (launches) *launches = k + 3;
  return hipGetLastError();
}

hipError_t launch_parts_plan(const PartsPlanArgs& a, hipStream_t st, uint32_t* launches) {
  uint32_t k = 1;
  const uint64_t words = a.n_lists > 16 + kKeys ? a.n_lists : 16 + kKeys;
  hipLaunchKernelGGL(k_parts_init, dim3(grid256(words)), dim3(256), 0, st, a);
  if (a.action_list) {
    hipLaunchKernelGGL(k_parts_mark, dim3(grid256(a.n_actions)), dim3(256), 0, st, a);
    ++k;
  }
  hipLaunchKernelGGL(k_parts_measure, dim3(grid256(a.n_lists)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_parts_scan, dim3(1), dim3(kScanThreads), 0, st, a);
  hipLaunchKernelGGL(k_parts_scatter, dim3(grid256(a.n_lists)), dim3(256), 0, st, a);
  if (launches) *launches = k + 3;
  return hipGetLastError();
}

hipError_t launch_digest_parts_planned(const PartsPlanArgs& a, hipStream_t st) {
  uint8_t* dst = a.action_list ? a.table : a.out;
  hipLaunchKernelGGL(k_digest_parts_planned, dim3(grid256(a.n_lists)), dim3(256), 0, st, a.arena, a.part_off,
                     a.part_len, a.begin, a.order, a.n_lists, dst, a.err);
  return hipGetLastError();
}

hipError_t launch_parts_fill(const PartsPlanArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_parts_fill, dim3(grid256(a.n_actions)), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace msha
