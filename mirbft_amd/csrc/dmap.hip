// Device digest maps (gfx950 only): the kernels behind msha_dmap_add_device, _find_device
// and _clear_device (include/mirsha.h "Device digest maps"). What a step does and why the
// answer does not depend on the table: dmap.hpp.
//
// An add is seven kernels on the caller's stream, every dependency a kernel boundary, no
// memset, no host wait, and no workgroup waits for another. The first three are group.hip's
// (k_group_init, _insert, _resolve) on the call's own table: they leave first[i] and the
// members at each leader. Then, here:
//   k_dmap_find      a lane a slot, leaders only: dmap::find_probe over the map's table,
//                    READ-ONLY. The table's words are read by agent-scope relaxed atomic
//                    loads; the stored keys and counts by plain loads (nothing writes them
//                    in this launch). Per leader: id or NEW, where the walk stopped, the
//                    count before. Per tile, by wave ballots: new leaders, crossing leaders.
//   k_dmap_scan      ONE workgroup: group::scan_walk over both totals -> the leaders of
//                    each kind before each tile, `added`, `crossed`, and the decision
//                    full = entries + added > max_keys.
//   k_dmap_commit    nothing when full. A new leader numbers itself, writes its key and
//                    count at its id and claims a table position from where its find
//                    stopped (compare-and-swap EMPTY -> id, agent scope; no compare of
//                    keys: dmap.hpp). An existing leader stores its count: it is the only
//                    lane of the call with that key. Crossing leaders write their slot at
//                    base + rank; a tile's largest (after, ~id) by one 64-bit max.
//   k_dmap_fill      d_id, d_before, d_after from the leader's scratch; one thread writes
//                    the eight result words and entries += added.
// k_dmap_lookup (find_device) and k_dmap_clear (clear_device) are one launch each.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mirsha.h"
#include "dmap.hpp"
#include "kernels.hpp"

namespace msha {

namespace {

namespace gp = group;
namespace dm = dmap;

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

__device__ __forceinline__ void store_granule(uint8_t* p, const parts::Granule& g) {
  *reinterpret_cast<uint4*>(p) = make_uint4(g.d[0], g.d[1], g.d[2], g.d[3]);
}

// Slot s's key, from the caller's arrays.
__device__ __forceinline__ gp::Key slot_key(const DmapArgs& a, uint64_t s) {
  gp::Key k;
  k.scope = a.scope ? a.scope[s] : 0u;
  k.lo = load_granule(a.digests + 32u * s);
  k.hi = load_granule(a.digests + 32u * s + 16u);
  return k;
}

// Entry e's key, from the map's key store.
__device__ __forceinline__ gp::Key stored_key(const DmapArgs& a, uint32_t e) {
  gp::Key k;
  k.scope = a.key_scope[e];
  k.lo = load_granule(a.key_digests + 32ull * e);
  k.hi = load_granule(a.key_digests + 32ull * e + 16u);
  return k;
}

__device__ __forceinline__ gp::Placement placement(const DmapArgs& a) {
  gp::Placement pl;
  pl.seed = a.seed;
  pl.mask = (uint32_t)(a.capacity - 1);
  pl.force_home = a.force_home;
  pl.force_at = a.force_at;
  return pl;
}

// The read-only walk for key k.
__device__ __forceinline__ dm::Found walk(const DmapArgs& a, const gp::Key& k) {
  const gp::Placement pl = placement(a);
  return dm::find_probe(
      gp::home(pl, k), pl.mask,
      [&](uint32_t p) { return __hip_atomic_load(&a.table[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
      [&](uint32_t e) { return gp::same(k, stored_key(a, e)); });
}

// What a leader brings to commit, as find left it.
struct Lead {
  bool leads = false;
  uint32_t id = dm::kNew, before = 0, after = 0;
};
__device__ __forceinline__ Lead load_lead(const DmapArgs& a, uint64_t i) {
  Lead l;
  l.leads = i < a.n && a.first[i] == (uint32_t)i;
  if (l.leads) {
    l.id = a.lead_id[i];
    l.before = a.lead_before[i];
    l.after = dm::sat_add(l.before, a.members[i]);
  }
  return l;
}

__global__ __launch_bounds__(dm::kTile) void k_dmap_find(DmapArgs a) {
  __shared__ uint32_t w_new[dm::kTileWaves], w_cross[dm::kTileWaves];
  const uint32_t t = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * dm::kTile + t;
  const bool leads = i < a.n && a.first[i] == (uint32_t)i;
  bool is_new = false, crosses = false;
  if (leads) {
    const dm::Found f = walk(a, slot_key(a, i));
    is_new = f.id == dm::kNew;
    const uint32_t before = is_new ? 0u : a.count[f.id];
    a.lead_id[i] = f.id;
    a.lead_pos[i] = f.pos;
    a.lead_before[i] = before;
    crosses = dm::crossed(a.threshold, before, dm::sat_add(before, a.members[i]));
  }
  const uint64_t m_new = __ballot(is_new), m_cross = __ballot(crosses);
  if (wave_lane() == 0) {
    w_new[t >> 6] = (uint32_t)__popcll(m_new);
    w_cross[t >> 6] = (uint32_t)__popcll(m_cross);
  }
  __syncthreads();
  if (t == 0) {
    uint32_t s_new = 0, s_cross = 0;
#pragma unroll
    for (uint32_t w = 0; w < dm::kTileWaves; ++w) {
      s_new += w_new[w];
      s_cross += w_cross[w];
    }
    a.tot_new[blockIdx.x] = s_new;
    a.tot_cross[blockIdx.x] = s_cross;
  }
}

__global__ __launch_bounds__(gp::kScanThreads) void k_dmap_scan(DmapArgs a) {
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

  const uint64_t tiles = gp::tiles(a.n);
  const uint64_t added = gp::scan_walk(
      tiles, t, [&](uint64_t k) { return a.tot_new[k]; }, prefix,
      [&](uint64_t k, uint32_t before) { a.tot_new[k] = before; });
  const uint64_t crossed = gp::scan_walk(
      tiles, t, [&](uint64_t k) { return a.tot_cross[k]; }, prefix,
      [&](uint64_t k, uint32_t before) { a.tot_cross[k] = before; });
  if (t == 0) {
    a.head[dm::kHeadAdded] = added;
    a.head[dm::kHeadCrossed] = crossed;
    a.head[dm::kHeadFull] = dm::refuse(a.head[dm::kHeadEntries], added, a.max_keys) ? 1 : 0;
  }
}

__global__ __launch_bounds__(dm::kTile) void k_dmap_commit(DmapArgs a) {
  __shared__ uint64_t s_new[dm::kTileWaves], s_cross[dm::kTileWaves], s_best[dm::kTileWaves];
  if (a.head[dm::kHeadFull]) return;  // the whole grid alike: nothing of the map is written
  const uint32_t t = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * dm::kTile + t;
  const Lead l = load_lead(a, i);
  const bool is_new = l.leads && l.id == dm::kNew;
  const bool crosses = l.leads && dm::crossed(a.threshold, l.before, l.after);
  const uint64_t m_new = __ballot(is_new), m_cross = __ballot(crosses);
  if (wave_lane() == 0) {
    s_new[t >> 6] = m_new;
    s_cross[t >> 6] = m_cross;
  }
  __syncthreads();

  uint64_t best = 0;
  if (l.leads) {
    uint64_t ballots[dm::kTileWaves];
    uint32_t id = l.id;
    if (is_new) {
#pragma unroll
      for (uint32_t w = 0; w < dm::kTileWaves; ++w) ballots[w] = s_new[w];
      // entries + added <= max_keys (not full): id is inside the key store
      id = dm::new_id(a.head[dm::kHeadEntries], (uint64_t)a.tot_new[blockIdx.x] + gp::rank_in_tile(ballots, t >> 6, wave_lane()));
      const gp::Key k = slot_key(a, i);
      a.key_scope[id] = k.scope;
      store_granule(a.key_digests + 32ull * id, k.lo);
      store_granule(a.key_digests + 32ull * id + 16u, k.hi);
      a.lead_id[i] = id;
      (void)dm::insert_probe(id, a.lead_pos[i], (uint32_t)(a.capacity - 1),
                             [&](uint32_t p, uint32_t me) { return atomicCAS(&a.table[p], dm::kEmpty, me); });
    }
    a.count[id] = l.after;
    if (crosses) {
#pragma unroll
      for (uint32_t w = 0; w < dm::kTileWaves; ++w) ballots[w] = s_cross[w];
      const uint64_t r = (uint64_t)a.tot_cross[blockIdx.x] + gp::rank_in_tile(ballots, t >> 6, wave_lane());
      if (r < a.crossed_cap) a.crossed_slot[r] = (uint32_t)i;
    }
    best = gp::best_key(l.after, id);
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
    for (uint32_t w = 0; w < dm::kTileWaves; ++w) best = s_best[w] > best ? s_best[w] : best;
    if (best != 0)  // a tile without a leader has nothing to offer
      atomicMax(reinterpret_cast<unsigned long long*>(a.best), (unsigned long long)best);
  }
}

__global__ __launch_bounds__(dm::kTile) void k_dmap_fill(DmapArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * dm::kTile + threadIdx.x;
  const bool full = a.head[dm::kHeadFull] != 0;
  if (i < a.n) {
    const uint32_t f = a.first[i];
    const uint32_t before = a.lead_before[f];
    a.id[i] = full ? dm::kNoId : a.lead_id[f];
    if (a.before) a.before[i] = before;
    if (a.after) a.after[i] = dm::sat_add(before, a.members[f]);
  }
  if (i == 0) {  // no other thread of this launch reads or writes `entries`
    uint64_t r[8];
    dm::result_words(a.n, a.head[dm::kHeadEntries], a.head[dm::kHeadAdded], full, a.head[dm::kHeadCrossed], a.crossed_cap,
                     *a.best, r);
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) a.result[k] = r[k];
    a.head[dm::kHeadEntries] = r[1];
  }
}

__global__ __launch_bounds__(dm::kTile) void k_dmap_lookup(DmapArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * dm::kTile + threadIdx.x;
  if (i >= a.n) return;
  const dm::Found f = walk(a, slot_key(a, i));
  const bool found = f.id != dm::kNew;
  a.id[i] = found ? f.id : dm::kNoId;
  if (a.after) a.after[i] = found ? a.count[f.id] : 0u;
}

__global__ __launch_bounds__(dm::kTile) void k_dmap_clear(DmapArgs a) {
  const uint64_t q = (uint64_t)blockIdx.x * dm::kTile + threadIdx.x;  // four entries a thread
  // capacity is a power of two, at least 64
  if (q < a.capacity / 4) reinterpret_cast<uint4*>(a.table)[q] = make_uint4(dm::kEmpty, dm::kEmpty, dm::kEmpty, dm::kEmpty);
  if (q < dm::kHeadWords) a.head[q] = 0;
  // a vote map's masks (none on a plain map): every key's set of voters empty
  if (q < a.mask_quads) reinterpret_cast<uint4*>(a.masks)[q] = make_uint4(0, 0, 0, 0);
}

// n <= 2^30 (the host's bound): at most 2^22 tiles
unsigned tile_grid(const DmapArgs& a) { return (unsigned)gp::tiles(a.n); }

}  // namespace

hipError_t launch_dmap_find(const DmapArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_dmap_find, dim3(tile_grid(a)), dim3(dm::kTile), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_dmap_scan(const DmapArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_dmap_scan, dim3(1), dim3(gp::kScanThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_dmap_commit(const DmapArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_dmap_commit, dim3(tile_grid(a)), dim3(dm::kTile), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_dmap_fill(const DmapArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_dmap_fill, dim3(tile_grid(a)), dim3(dm::kTile), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_dmap_lookup(const DmapArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_dmap_lookup, dim3(tile_grid(a)), dim3(dm::kTile), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_dmap_clear(const DmapArgs& a, hipStream_t st) {
  // capacity <= 2^31: at most 2^21 workgroups for the table; the masks of a vote map are
  // at most 2^30 keys of 32 words, 2^33 quads: 2^25 workgroups. The larger range decides.
  const uint64_t quads = a.capacity / 4 > a.mask_quads ? a.capacity / 4 : a.mask_quads;
  const unsigned grid = (unsigned)((quads + dm::kTile - 1) / dm::kTile);
  hipLaunchKernelGGL(k_dmap_clear, dim3(grid), dim3(dm::kTile), 0, st, a);
  return hipGetLastError();
}

}  // namespace msha
