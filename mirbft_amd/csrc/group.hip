// msha_group_digests_device (gfx950 only): digests grouped by value, the answer left in
// HBM in order of first occurrence (include/mirsha.h "Digests grouped by value on the
// GPU"). What a step does and why the answer does not depend on the table: group.hpp.
//
// Six kernels on the caller's stream, every dependency a kernel boundary, no memset, no
// host wait, and no workgroup waits for another:
//   k_group_init     table entries EMPTY, the leaders' counters and the best word 0
//                    (16-byte stores).
//   k_group_insert   a lane a slot: group::probe. The table's entries are the only words
//                    workgroups exchange inside this launch, and they are touched by
//                    agent-scope atomics alone (relaxed load, compare-and-swap, min); the
//                    digest rows and scopes are launch inputs, read by plain 16-byte and
//                    4-byte loads. The lane stores where it stopped. Lanes of a wave with
//                    an earlier lane's hash go second (a matter of time, not of result).
//   k_group_resolve  first[i] = table[pos[i]] -> d_first; the tile's leaders by wave
//                    ballots -> totals; the members joined a leader in an LDS tile table
//                    (a wave of one leader: one LDS add), then one global add a leader
//                    and tile: a key that every slot holds costs a tile one atomic.
//   k_group_scan     ONE workgroup: the tile totals -> the leaders before each tile, and
//                    `groups` (group::scan_walk). tiles(n) = n / 256 words, not n.
//   k_group_rank     a leader's id = its tile's base + its rank among the tile's leaders;
//                    id, and below group_cap d_group_first and d_group_count; the tile's
//                    largest (count, ~id) by one 64-bit max into the workspace.
//   k_group_fill     d_group[i] = id[first[i]], d_members[i] = count[first[i]]; one thread
//                    writes the five result words.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mirsha.h"
#include "group.hpp"
#include "kernels.hpp"

namespace msha {

namespace {

namespace gp = group;

__device__ __forceinline__ uint32_t wave_lane() { return threadIdx.x & 63u; }

// A lane's value, the lane wave-uniform (found by a ballot): v_readlane.
__device__ __forceinline__ uint32_t lane_value(uint32_t v, int lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}

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

__device__ __forceinline__ gp::Key load_key(const GroupArgs& a, uint64_t s) {
  gp::Key k;
  k.scope = a.scope ? a.scope[s] : 0u;
  k.lo = load_granule(a.digests + 32u * s);
  k.hi = load_granule(a.digests + 32u * s + 16u);
  return k;
}

__global__ __launch_bounds__(gp::kTile) void k_group_init(GroupArgs a) {
  const uint64_t q = (uint64_t)blockIdx.x * gp::kTile + threadIdx.x;  // four entries a thread
  // capacity is a multiple of 4; the counters' array is laid out in whole 256 bytes
  if (q < a.capacity / 4) reinterpret_cast<uint4*>(a.table)[q] = make_uint4(gp::kEmpty, gp::kEmpty, gp::kEmpty, gp::kEmpty);
  if (q < (a.n + 3) / 4) reinterpret_cast<uint4*>(a.count)[q] = make_uint4(0, 0, 0, 0);
  if (q == 0) a.head[gp::kHeadBest] = 0;
}

__global__ __launch_bounds__(gp::kTile) void k_group_insert(GroupArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * gp::kTile + threadIdx.x;
  const bool valid = i < a.n;
  gp::Key k{};
  if (valid) k = load_key(a, i);
  gp::Placement pl;
  pl.seed = a.seed;
  pl.mask = (uint32_t)(a.capacity - 1);
  pl.force_home = a.force_home;
  pl.force_at = a.force_at;
  const uint64_t hashed = gp::hash(pl.seed, k);
  const uint32_t h_lo = (uint32_t)hashed, h_hi = (uint32_t)(hashed >> 32);

  // WHEN a lane probes, never what it does: the lanes of a wave whose hash equals that of
  // an earlier lane wait until that lane is through, and then run the same probe with
  // the same full compare. While a table is still empty every resident lane of a hot key
  // sees EMPTY and would claim: one compare-and-swap a lane on one word (3.7 ms for one
  // group of 2^20, profiles/group/README.md). The earlier lane has the smaller slot, so
  // the lanes behind it find its claim, compare, and have nothing to lower. The first
  // kElect distinct hashes of a wave are looked at; a hash is only a hint here.
  constexpr int kElect = 4;
  bool later = false;
  uint64_t todo = __ballot(valid);
#pragma unroll
  for (int r = 0; r < kElect; ++r) {
    if (todo == 0) break;  // wave-uniform
    const int l = __ffsll((unsigned long long)todo) - 1;
    const bool like =
        valid && h_lo == lane_value(h_lo, l) && h_hi == lane_value(h_hi, l);
    if (like && (int)wave_lane() != l) later = true;
    todo &= ~__ballot(like);
  }

  const auto insert = [&] {
    a.pos[i] = gp::probe(
        (uint32_t)i, gp::home_of(pl, hashed), pl.mask,
        [&](uint32_t p) { return __hip_atomic_load(&a.table[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
        [&](uint32_t p, uint32_t me) { return atomicCAS(&a.table[p], gp::kEmpty, me); },
        [&](uint32_t p, uint32_t me) { atomicMin(&a.table[p], me); },
        [&](uint32_t j) { return gp::same(k, load_key(a, j)); });
  };
  if (valid && !later) insert();
  // behind the first: program order in one wave, one word, agent-scope atomics (the empty
  // statement keeps the compiler from folding the two rounds into one)
  asm volatile("; k_group_insert second round" ::: "memory");
  if (valid && later) insert();
}

__global__ __launch_bounds__(gp::kTile) void k_group_resolve(GroupArgs a) {
  __shared__ uint32_t t_key[gp::kTileSlots], t_cnt[gp::kTileSlots];
  __shared__ uint32_t w_leaders[gp::kTileWaves];
  const uint32_t t = threadIdx.x;
  for (uint32_t j = t; j < gp::kTileSlots; j += gp::kTile) {
    t_key[j] = gp::kEmpty;
    t_cnt[j] = 0;
  }
  __syncthreads();

  const uint64_t i = (uint64_t)blockIdx.x * gp::kTile + t;
  const bool valid = i < a.n;
  uint32_t first = gp::kEmpty;
  if (valid) {
    first = a.table[a.pos[i]];
    a.first[i] = first;
  }
  const uint64_t leads = __ballot(valid && first == (uint32_t)i);
  if (wave_lane() == 0) w_leaders[t >> 6] = (uint32_t)__popcll(leads);

  const auto slot_of = [&](uint32_t f) {
    return gp::tile_slot(
        f, [&](uint32_t h) { return t_key[h]; }, [&](uint32_t h, uint32_t me) { return atomicCAS(&t_key[h], gp::kEmpty, me); });
  };
  // a wave whose slots all follow one leader (a clean quorum, one EpochChange digest
  // acknowledged N^2 times) adds once; slots ascend with the lane, so lane 0 is valid
  // whenever any lane is
  const uint32_t f0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)first);
  const uint64_t in = __ballot(valid), like0 = __ballot(valid && first == f0);
  if (like0 == in) {
    if (wave_lane() == 0 && in != 0) atomicAdd(&t_cnt[slot_of(f0)], (uint32_t)__popcll(in));
  } else if (valid) {
    atomicAdd(&t_cnt[slot_of(first)], 1u);
  }
  __syncthreads();

  for (uint32_t j = t; j < gp::kTileSlots; j += gp::kTile)
    if (t_key[j] != gp::kEmpty) atomicAdd(&a.count[t_key[j]], t_cnt[j]);
  if (t == 0) {
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t w = 0; w < gp::kTileWaves; ++w) sum += w_leaders[w];
    a.totals[blockIdx.x] = sum;
  }
}

__global__ __launch_bounds__(gp::kScanThreads) void k_group_scan(GroupArgs a) {
  constexpr uint32_t kWaves = gp::kScanThreads / 64;
  __shared__ uint32_t wsum[kWaves];
  const uint32_t t = threadIdx.x;

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

  const uint64_t groups = gp::scan_walk(
      gp::tiles(a.n), t, [&](uint64_t k) { return a.totals[k]; }, prefix,
      [&](uint64_t k, uint32_t before) { a.totals[k] = before; });
  if (t == 0) a.head[gp::kHeadGroups] = groups;
}

__global__ __launch_bounds__(gp::kTile) void k_group_rank(GroupArgs a) {
  __shared__ uint64_t s_leads[gp::kTileWaves], s_best[gp::kTileWaves];
  const uint32_t t = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * gp::kTile + t;
  const bool leads = i < a.n && a.first[i] == (uint32_t)i;
  const uint64_t m = __ballot(leads);
  if (wave_lane() == 0) s_leads[t >> 6] = m;
  __syncthreads();

  uint64_t best = 0;
  if (leads) {
    uint64_t ballots[gp::kTileWaves];
#pragma unroll
    for (uint32_t w = 0; w < gp::kTileWaves; ++w) ballots[w] = s_leads[w];
    const uint32_t id = a.totals[blockIdx.x] + gp::rank_in_tile(ballots, t >> 6, wave_lane());
    const uint32_t c = a.count[i];
    a.id[i] = id;
    if (id < a.group_cap) {
      a.group_first[id] = (uint32_t)i;
      a.group_count[id] = c;
    }
    best = gp::best_key(c, id);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint64_t o = __shfl_xor((unsigned long long)best, d);
    best = o > best ? o : best;
  }
  if (wave_lane() == 0) s_best[t >> 6] = best;
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (uint32_t w = 0; w < gp::kTileWaves; ++w) best = s_best[w] > best ? s_best[w] : best;
    if (best != 0)  // a tile without a leader has nothing to offer
      atomicMax(reinterpret_cast<unsigned long long*>(&a.head[gp::kHeadBest]), (unsigned long long)best);
  }
}

__global__ __launch_bounds__(gp::kTile) void k_group_fill(GroupArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * gp::kTile + threadIdx.x;
  if (i < a.n) {
    const uint32_t f = a.first[i];
    a.group[i] = a.id[f];
    if (a.members) a.members[i] = a.count[f];
  }
  if (i == 0) {
    uint64_t r[5];
    gp::result_words(a.n, a.head[gp::kHeadGroups], a.group_cap, a.head[gp::kHeadBest], r);
#pragma unroll
    for (uint32_t k = 0; k < 5; ++k) a.result[k] = r[k];
  }
}

// n <= 2^30 (the host's bound): at most 2^22 tiles
unsigned tile_grid(const GroupArgs& a) { return (unsigned)gp::tiles(a.n); }

}  // namespace

hipError_t launch_group_init(const GroupArgs& a, hipStream_t st) {
  // capacity >= 2 n: the table's quarter covers the counters' quarter; at most 2^21 workgroups
  const unsigned grid = (unsigned)((a.capacity / 4 + gp::kTile - 1) / gp::kTile);
  hipLaunchKernelGGL(k_group_init, dim3(grid), dim3(gp::kTile), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_group_insert(const GroupArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_group_insert, dim3(tile_grid(a)), dim3(gp::kTile), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_group_resolve(const GroupArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_group_resolve, dim3(tile_grid(a)), dim3(gp::kTile), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_group_scan(const GroupArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_group_scan, dim3(1), dim3(gp::kScanThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_group_rank(const GroupArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_group_rank, dim3(tile_grid(a)), dim3(gp::kTile), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_group_fill(const GroupArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_group_fill, dim3(tile_grid(a)), dim3(gp::kTile), 0, st, a);
  return hipGetLastError();
}

}  // namespace msha
