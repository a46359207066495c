// Vote maps (gfx950 only): the kernels behind msha_dmap_vote_device and
// msha_dmap_find_votes_device (include/mirsha.h "Device digest maps that count voters").
// What a step does and why the answer does not depend on the tables or on the order the
// lanes ran in: dmap_vote.hpp, on top of dmap.hpp.
//
// A vote is ten kernels on the caller's stream, every dependency a kernel boundary, no
// memset, no host wait, and no workgroup waits for another. The first three are group.hip's
// (k_group_init, _insert, _resolve) on the call's own table: they leave first[i]. Then, here:
//   k_vote_find      as k_dmap_find without the totals: leaders walk the map's table
//                    READ-ONLY (agent-scope relaxed atomic loads of the table's words,
//                    plain loads of the stored keys and counts) and leave id or NEW, where
//                    the walk stopped and the count before. The same launch empties the
//                    pair table and zeroes fresh[]: nothing before it reads either.
//   k_vote_pair      a lane a slot with a voter in range: group::probe on the pair table,
//                    keyed by (first[i], voter[i]); the table's entries are touched by
//                    agent-scope atomics alone (relaxed load, compare-and-swap, min).
//                    Lanes of a wave with an earlier lane's pair go second (a matter of
//                    time, not of result), as in k_group_insert.
//   k_vote_count     a lane a slot. A pair leader (its entry holds its slot) reads its
//                    key's id at the key's leader and, for a held key, the one mask word
//                    by a plain load (nothing writes masks in this launch): counted[i].
//                    The counted slots of a key are joined in an LDS tile table
//                    (group::tile_slot, as k_group_resolve joins members) and go to
//                    fresh[first] by one global add a key and tile. Tile totals of
//                    counted, repeats and bad voters by wave ballots.
//   k_vote_totals    leaders: after = before + fresh; new and crossing leaders a tile, by
//                    wave ballots (what k_dmap_find leaves for an add).
//   k_vote_scan      ONE workgroup: group::scan_walk over the two totals as k_dmap_scan, the
//                    decision full, and the sums of the three other totals.
//   k_vote_commit    as k_dmap_commit with fresh where that has the members: nothing when
//                    full. Masks are not touched: a new id's mask is empty already.
//   k_vote_fill      d_id, d_counted, d_before, d_after, the eleven result words and
//                    entries += added; and, unless full, a counted slot sets its voter's bit
//                    in its key's mask: atomicOr, 32-bit, agent scope, since several pairs
//                    may share a word. A launch behind commit, so the new ids are there.
// k_vote_lookup (find_votes_device) is one launch, read-only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mirsha.h"
#include "dmap_vote.hpp"
#include "kernels.hpp"

namespace msha {

namespace {

namespace gp = group;
namespace dm = dmap;
namespace dv = dmap_vote;

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

__device__ __forceinline__ void store_granule(uint8_t* p, const parts::Granule& g) {
  *reinterpret_cast<uint4*>(p) = make_uint4(g.d[0], g.d[1], g.d[2], g.d[3]);
}

// Slot s's key, from the caller's arrays.
__device__ __forceinline__ gp::Key slot_key(const DmapVoteArgs& a, uint64_t s) {
  gp::Key k;
  k.scope = a.scope ? a.scope[s] : 0u;
  k.lo = load_granule(a.digests + 32u * s);
  k.hi = load_granule(a.digests + 32u * s + 16u);
  return k;
}

// Entry e's key, from the map's key store.
__device__ __forceinline__ gp::Key stored_key(const DmapVoteArgs& a, uint32_t e) {
  gp::Key k;
  k.scope = a.key_scope[e];
  k.lo = load_granule(a.key_digests + 32ull * e);
  k.hi = load_granule(a.key_digests + 32ull * e + 16u);
  return k;
}

// The read-only walk for key k over the map's table.
__device__ __forceinline__ dm::Found walk(const DmapVoteArgs& a, const gp::Key& k) {
  gp::Placement pl;
  pl.seed = a.seed;
  pl.mask = (uint32_t)(a.capacity - 1);
  pl.force_home = a.force_home;
  pl.force_at = a.force_at;
  return dm::find_probe(
      gp::home(pl, k), pl.mask,
      [&](uint32_t p) { return __hip_atomic_load(&a.table[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
      [&](uint32_t e) { return gp::same(k, stored_key(a, e)); });
}

// The sum of a per-lane flag over the tile, to out[blockIdx.x], through the waves' ballots.
// Every thread of the workgroup calls it; w is kTileWaves words of LDS of the caller's.
__device__ __forceinline__ void tile_total(bool flag, uint32_t* w, uint32_t* out) {
  const uint64_t m = __ballot(flag);
  if (wave_lane() == 0) w[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < dm::kTileWaves; ++k) s += w[k];
    out[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(dm::kTile) void k_vote_find(DmapVoteArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * dm::kTile + threadIdx.x;
  // four entries a thread: the pair table has at most max(4 n, 64) entries and the grid at
  // least max(n, 256) threads; fresh[] is laid out in whole 256 bytes
  if (i < a.pair_capacity / 4)
    reinterpret_cast<uint4*>(a.pair_table)[i] = make_uint4(gp::kEmpty, gp::kEmpty, gp::kEmpty, gp::kEmpty);
  if (i < (a.n + 3) / 4) reinterpret_cast<uint4*>(a.fresh)[i] = make_uint4(0, 0, 0, 0);
  if (i < a.n && a.first[i] == (uint32_t)i) {
    const dm::Found f = walk(a, slot_key(a, i));
    a.lead_id[i] = f.id;
    a.lead_pos[i] = f.pos;
    a.lead_before[i] = f.id == dm::kNew ? 0u : a.count[f.id];
  }
}

__global__ __launch_bounds__(dm::kTile) void k_vote_pair(DmapVoteArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * dm::kTile + threadIdx.x;
  uint32_t v = 0, f = 0;
  bool valid = i < a.n;
  if (valid) {
    v = a.voter[i];
    f = a.first[i];
    valid = dv::in_range(v, a.max_voters);  // a slot whose voter is out of range does not enter; pair_pos[i] is not read then
  }
  gp::Placement pl;
  pl.seed = a.pair_seed;
  pl.mask = (uint32_t)(a.pair_capacity - 1);
  pl.force_home = a.pair_force_home;
  pl.force_at = a.pair_force_at;

  // WHEN a lane probes, never what it does, as in k_group_insert: the lanes of a wave that
  // hold the pair of an earlier lane wait until that lane is through. A sender that repeats
  // one vote over and over is the case this map exists for, and without this every resident
  // lane of the pair would compare-and-swap one word of the empty table. The first kElect
  // distinct pairs of a wave are looked at.
  constexpr int kElect = 4;
  bool later = false;
  uint64_t todo = __ballot(valid);
#pragma unroll
  for (int r = 0; r < kElect; ++r) {
    if (todo == 0) break;  // wave-uniform
    const int l = __ffsll((unsigned long long)todo) - 1;
    const bool like = valid && dv::pair_same(f, v, lane_value(f, l), lane_value(v, l));
    if (like && (int)wave_lane() != l) later = true;
    todo &= ~__ballot(like);
  }

  const auto insert = [&] {
    // at most n pairs enter a table of at least 2 n positions: the probe ends
    a.pair_pos[i] = gp::probe(
        (uint32_t)i, gp::home_of(pl, dv::pair_hash(pl.seed, f, v)), pl.mask,
        [&](uint32_t p) { return __hip_atomic_load(&a.pair_table[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
        [&](uint32_t p, uint32_t me) { return atomicCAS(&a.pair_table[p], gp::kEmpty, me); },
        [&](uint32_t p, uint32_t me) { atomicMin(&a.pair_table[p], me); },
        [&](uint32_t j) { return dv::pair_same(f, v, a.first[j], a.voter[j]); });  // j: a slot that entered, below n
  };
  if (valid && !later) insert();
  // behind the first: program order in one wave, one word, agent-scope atomics (the empty
  // statement keeps the compiler from folding the two rounds into one)
  asm volatile("; k_vote_pair second round" ::: "memory");
  if (valid && later) insert();
}

__global__ __launch_bounds__(dm::kTile) void k_vote_count(DmapVoteArgs a) {
  __shared__ uint32_t t_key[gp::kTileSlots], t_cnt[gp::kTileSlots];
  __shared__ uint32_t w_counted[dm::kTileWaves], w_repeats[dm::kTileWaves], w_bad[dm::kTileWaves];
  const uint32_t t = threadIdx.x;
  for (uint32_t j = t; j < gp::kTileSlots; j += dm::kTile) {
    t_key[j] = gp::kEmpty;
    t_cnt[j] = 0;
  }
  __syncthreads();

  const uint64_t i = (uint64_t)blockIdx.x * dm::kTile + t;
  const bool valid = i < a.n;
  bool good = false, counts = false;
  uint32_t first = gp::kEmpty;
  if (valid) {
    const uint32_t v = a.voter[i];
    good = dv::in_range(v, a.max_voters);
    first = a.first[i];
    if (good) {
      const bool pair_leader = a.pair_table[a.pair_pos[i]] == (uint32_t)i;
      uint32_t word = 0;
      if (pair_leader) {
        const uint32_t id = a.lead_id[first];
        // id < entries <= max_keys, and v < max_voters: inside the mask store
        if (id != dm::kNew) word = a.masks[(uint64_t)id * a.mask_words + dv::mask_word(v)];
      }
      counts = dv::counted(pair_leader, word, v);
    }
    a.counted[i] = counts ? 1u : 0u;
  }
  if (counts) {
    const uint32_t h = gp::tile_slot(
        first, [&](uint32_t s) { return t_key[s]; },
        [&](uint32_t s, uint32_t me) { return atomicCAS(&t_key[s], gp::kEmpty, me); });
    atomicAdd(&t_cnt[h], 1u);
  }
  __syncthreads();
  for (uint32_t j = t; j < gp::kTileSlots; j += dm::kTile)
    if (t_key[j] != gp::kEmpty) atomicAdd(&a.fresh[t_key[j]], t_cnt[j]);

  tile_total(counts, w_counted, a.tot_counted);
  tile_total(valid && good && !counts, w_repeats, a.tot_repeats);
  tile_total(valid && !good, w_bad, a.tot_bad);
}

// What a leader brings to totals and commit.
struct Lead {
  bool leads = false;
  uint32_t id = dm::kNew, before = 0, after = 0;
};
__device__ __forceinline__ Lead load_lead(const DmapVoteArgs& a, uint64_t i) {
  Lead l;
  l.leads = i < a.n && a.first[i] == (uint32_t)i;
  if (l.leads) {
    l.id = a.lead_id[i];
    l.before = a.lead_before[i];
    l.after = l.before + a.fresh[i];  // at most max_voters
  }
  return l;
}

__global__ __launch_bounds__(dm::kTile) void k_vote_totals(DmapVoteArgs a) {
  __shared__ uint32_t w_new[dm::kTileWaves], w_cross[dm::kTileWaves];
  const uint64_t i = (uint64_t)blockIdx.x * dm::kTile + threadIdx.x;
  const Lead l = load_lead(a, i);
  tile_total(l.leads && l.id == dm::kNew, w_new, a.tot_new);
  tile_total(l.leads && dm::crossed(a.threshold, l.before, l.after), w_cross, a.tot_cross);
}

__global__ __launch_bounds__(gp::kScanThreads) void k_vote_scan(DmapVoteArgs a) {
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
  // the three sums alone: nobody ranks by these totals
  const auto sum = [&](const uint32_t* tot) {
    return gp::scan_walk(
        tiles, t, [&](uint64_t k) { return tot[k]; }, prefix, [](uint64_t, uint32_t) {});
  };
  const uint64_t counted = sum(a.tot_counted), repeats = sum(a.tot_repeats), bad = sum(a.tot_bad);
  if (t == 0) {
    a.head[dm::kHeadAdded] = added;
    a.head[dm::kHeadCrossed] = crossed;
    a.head[dm::kHeadFull] = dm::refuse(a.head[dm::kHeadEntries], added, a.max_keys) ? 1 : 0;
    a.vhead[dv::kHeadCounted] = counted;
    a.vhead[dv::kHeadRepeats] = repeats;
    a.vhead[dv::kHeadBad] = bad;
  }
}

__global__ __launch_bounds__(dm::kTile) void k_vote_commit(DmapVoteArgs a) {
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

__global__ __launch_bounds__(dm::kTile) void k_vote_fill(DmapVoteArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * dm::kTile + threadIdx.x;
  const bool full = a.head[dm::kHeadFull] != 0;
  if (i < a.n) {
    const uint32_t f = a.first[i];
    const uint32_t before = a.lead_before[f], c = a.counted[i];
    const uint32_t id = a.lead_id[f];  // numbered by commit, unless full
    a.id[i] = full ? dm::kNoId : id;
    if (a.counted_out) a.counted_out[i] = c;
    if (a.before) a.before[i] = before;
    if (a.after) a.after[i] = before + a.fresh[f];
    if (c && !full) {
      const uint32_t v = a.voter[i];  // counted: v < max_voters; not full: id < entries <= max_keys
      atomicOr(&a.masks[(uint64_t)id * a.mask_words + dv::mask_word(v)], dv::mask_bit(v));
    }
  }
  if (i == 0) {  // no other thread of this launch reads or writes `entries`
    uint64_t r[dv::kResultWords];
    dv::result_words(a.n, a.head[dm::kHeadEntries], a.head[dm::kHeadAdded], full, a.head[dm::kHeadCrossed], a.crossed_cap,
                     *a.best, a.vhead[dv::kHeadCounted], a.vhead[dv::kHeadRepeats], a.vhead[dv::kHeadBad], r);
#pragma unroll
    for (uint32_t k = 0; k < dv::kResultWords; ++k) a.result[k] = r[k];
    a.head[dm::kHeadEntries] = r[1];
  }
}

__global__ __launch_bounds__(dm::kTile) void k_vote_lookup(DmapVoteArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * dm::kTile + threadIdx.x;
  if (i >= a.n) return;
  const dm::Found f = walk(a, slot_key(a, i));
  const bool found = f.id != dm::kNew;
  const uint32_t v = a.voter[i];
  a.id[i] = found ? f.id : dm::kNoId;
  if (a.after) a.after[i] = found ? a.count[f.id] : 0u;
  uint32_t voted = 0;
  if (found && dv::in_range(v, a.max_voters))
    voted = (a.masks[(uint64_t)f.id * a.mask_words + dv::mask_word(v)] & dv::mask_bit(v)) != 0 ? 1u : 0u;
  a.counted_out[i] = voted;
}

// n <= 2^30 (the host's bound): at most 2^22 tiles
unsigned tile_grid(const DmapVoteArgs& a) { return (unsigned)gp::tiles(a.n); }

template <class Kernel>
hipError_t per_slot(Kernel k, const DmapVoteArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k, dim3(tile_grid(a)), dim3(dm::kTile), 0, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_vote_find(const DmapVoteArgs& a, hipStream_t st) { return per_slot(k_vote_find, a, st); }
hipError_t launch_vote_pair(const DmapVoteArgs& a, hipStream_t st) { return per_slot(k_vote_pair, a, st); }
hipError_t launch_vote_count(const DmapVoteArgs& a, hipStream_t st) { return per_slot(k_vote_count, a, st); }
hipError_t launch_vote_totals(const DmapVoteArgs& a, hipStream_t st) { return per_slot(k_vote_totals, a, st); }
hipError_t launch_vote_commit(const DmapVoteArgs& a, hipStream_t st) { return per_slot(k_vote_commit, a, st); }
hipError_t launch_vote_fill(const DmapVoteArgs& a, hipStream_t st) { return per_slot(k_vote_fill, a, st); }
hipError_t launch_vote_lookup(const DmapVoteArgs& a, hipStream_t st) { return per_slot(k_vote_lookup, a, st); }

hipError_t launch_vote_scan(const DmapVoteArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_vote_scan, dim3(1), dim3(gp::kScanThreads), 0, st, a);
  return hipGetLastError();
}

}  // namespace msha
