// Write jobs grouped by stream on the GPU (gfx950 only): the kernels of
// msha_dstreams_write_jobs_device (include/mirsha.h "Write jobs in call order";
// DESIGN.md "Device stream sets: write jobs").
//
// A stable LSD radix sort of (key, job index) pairs, stream_jobs.hpp, 8 bits a pass:
//   k_sjobs_hist     a workgroup per tile of kTileJobs jobs counts the pass's digits in
//                    LDS (the count does not depend on the order of the atomics) and
//                    stores them digit-major: counts[digit * n_tiles + tile].
//   k_sjobs_scan     a workgroup per DIGIT turns the digit's row of tile counts into its
//                    exclusive running sum, kScanThreads * kScanPer at a time with a
//                    carry (k_concat_scan's shape), and leaves the digit's total.
//   k_sjobs_scatter  a workgroup per tile again. Wave w ranks its kWaveJobs jobs in
//                    kRounds rounds of 64 consecutive jobs: eight ballots, one a digit
//                    bit, give a lane the lanes that share its digit; the peers below it
//                    are its rank in the round, the wave's count of that digit so far
//                    (LDS, this wave's row only) the rounds before. Then thread t, as
//                    digit t, adds up the waves' counts, the workgroup scans the 256
//                    digit totals for itself, and every job is stored at
//                    stream_jobs.hpp scatter_pos(). Nothing waits for another
//                    workgroup, so nothing can spin.
// The first pass reads the caller's ids (key = min(id, n), index = j); the others the
// pairs the pass before wrote, into the other buffer.
//   k_sjobs_rows     position p takes its job's offset and length; the last position
//                    raises kErrStreamRow when its key is n (those jobs sort last).
//   k_sjobs_begin    begin[t] = lower_bound(sorted keys, t) for t in [0, n], a lane an
//                    entry: balanced whatever the gaps between ids. begin[n] is the
//                    count of valid jobs, so k_dstream_write never reads a dropped one.
// Every store is guarded by the job count; every launch is on the caller's stream.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "stream_jobs.hpp"

namespace msha {

namespace {

namespace sj = sjobs;

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

// Job j of a pass: from the caller's ids in the first, from the pairs otherwise.
template <bool FIRST>
__device__ __forceinline__ uint2 load_pair(const StreamJobsArgs& a, const uint2* __restrict__ in, uint64_t j) {
  if (FIRST) return make_uint2(sj::clamp_key(a.job_stream[j], a.n_streams), (uint32_t)j);
  return in[j];
}

template <bool FIRST>
__global__ __launch_bounds__(sj::kThreads) void k_sjobs_hist(StreamJobsArgs a, const uint2* __restrict__ in,
                                                            uint32_t pass) {
  __shared__ uint32_t hist[sj::kDigits];
  const uint32_t t = threadIdx.x;
  const uint64_t tile = blockIdx.x, n_tiles = gridDim.x;
  hist[t] = 0;
  __syncthreads();
#pragma unroll
  for (uint32_t i = 0; i < sj::kTileJobs / sj::kThreads; ++i) {
    const uint64_t j = tile * sj::kTileJobs + i * sj::kThreads + t;
    if (j < a.n_jobs) atomicAdd(&hist[sj::digit(load_pair<FIRST>(a, in, j).x, pass)], 1u);
  }
  __syncthreads();
  a.counts[sj::count_index(t, tile, n_tiles)] = hist[t];
}

// Workgroup d: digit d's row of n_tiles counts -> its exclusive running sum, in place,
// kScanThreads * kScanPer at a time with a carry; the row's total behind the rows.
__global__ __launch_bounds__(sj::kScanThreads) void k_sjobs_scan(uint32_t* counts, uint64_t n_tiles) {
  __shared__ uint32_t wsum[sj::kScanThreads / 64];
  constexpr uint64_t kWidth = (uint64_t)sj::kScanThreads * sj::kScanPer;
  const uint32_t d = blockIdx.x;
  uint32_t* const row = counts + sj::count_index(d, 0, n_tiles);
  uint32_t carry = 0;
  for (uint64_t i0 = 0; i0 < n_tiles; i0 += kWidth) {
    const uint64_t i = i0 + (uint64_t)threadIdx.x * sj::kScanPer;
    uint32_t c[sj::kScanPer], s = 0;
#pragma unroll
    for (uint32_t j = 0; j < sj::kScanPer; ++j) {
      c[j] = i + j < n_tiles ? row[i + j] : 0;
      s += c[j];
    }
    const uint32_t inc = wave_scan(s);
    if (wave_lane() == 63) wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint32_t base = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < sj::kScanThreads / 64; ++w) {
      if (w < (threadIdx.x >> 6)) base += wsum[w];
      all += wsum[w];
    }
    uint32_t start = carry + base + inc - s;
#pragma unroll
    for (uint32_t j = 0; j < sj::kScanPer; ++j) {
      if (i + j < n_tiles) row[i + j] = start;
      start += c[j];
    }
    carry += all;
    __syncthreads();  // wsum is written again
  }
  if (threadIdx.x == 0) counts[sj::total_index(d, n_tiles)] = carry;
}

template <bool FIRST>
__global__ __launch_bounds__(sj::kThreads) void k_sjobs_scatter(StreamJobsArgs a, const uint2* __restrict__ in,
                                                               uint2* __restrict__ out, uint32_t pass) {
  // [wave][digit]: a wave's count of a digit, and the count of the tile's waves before it;
  // lower[digit]: the jobs of lower digits; tiles[digit]: the tile's entries of the scanned rows
  __shared__ uint32_t wcount[sj::kWaves][sj::kDigits];
  __shared__ uint32_t earlier[sj::kWaves][sj::kDigits];
  __shared__ uint32_t lower[sj::kDigits], tiles[sj::kDigits];
  __shared__ uint32_t wtotal[sj::kWaves];
  const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63u;
  const uint64_t tile = blockIdx.x, n_tiles = gridDim.x;
#pragma unroll
  for (uint32_t v = 0; v < sj::kWaves; ++v) wcount[v][t] = 0;
  __syncthreads();

  uint2 pr[sj::kRounds];
  uint32_t rank[sj::kRounds];
#pragma unroll
  for (uint32_t r = 0; r < sj::kRounds; ++r) {
    const uint64_t j = tile * sj::kTileJobs + sj::item_index(w, r, lane);
    const bool valid = j < a.n_jobs;
    pr[r] = valid ? load_pair<FIRST>(a, in, j) : make_uint2(0, 0);
    const uint32_t d = sj::digit(pr[r].x, pass);
    uint64_t bit_ballot[sj::kDigitBits];
#pragma unroll
    for (uint32_t b = 0; b < sj::kDigitBits; ++b) bit_ballot[b] = __ballot((d >> b) & 1u);
    const uint64_t peer_mask = sj::peers(d, bit_ballot, __ballot(valid));
    // the rounds before, read by every lane before the round's leaders add to it
    const uint32_t before = wcount[w][d];
    rank[r] = before + sj::lane_rank(peer_mask, lane);
    __syncthreads();
    if (valid && sj::leads(peer_mask, lane)) wcount[w][d] = before + sj::popcount64(peer_mask);
    __syncthreads();
  }

  // thread t is digit t: the waves' jobs of it, one wave after the other; the digits'
  // totals scanned by the workgroup, each for itself (256 values)
  uint32_t run = 0;
  tiles[t] = a.counts[sj::count_index(t, tile, n_tiles)];
#pragma unroll
  for (uint32_t v = 0; v < sj::kWaves; ++v) {
    earlier[v][t] = run;
    run += wcount[v][t];
  }
  const uint32_t total = a.counts[sj::total_index(t, n_tiles)];
  const uint32_t inc = wave_scan(total);
  if (lane == 63) wtotal[w] = inc;
  __syncthreads();
  uint32_t below = inc - total;
#pragma unroll
  for (uint32_t v = 0; v < sj::kWaves; ++v)
    if (v < w) below += wtotal[v];
  lower[t] = below;
  __syncthreads();

#pragma unroll
  for (uint32_t r = 0; r < sj::kRounds; ++r) {
    const uint64_t j = tile * sj::kTileJobs + sj::item_index(w, r, lane);
    if (j >= a.n_jobs) continue;
    const uint32_t d = sj::digit(pr[r].x, pass);
    const uint64_t pos = sj::scatter_pos(lower[d], tiles[d], earlier[w][d], rank[r]);
    if (pos < a.n_jobs) out[pos] = pr[r];  // always, when the counts are this pass's
  }
}

__global__ __launch_bounds__(256) void k_sjobs_rows(StreamJobsArgs a, const uint2* __restrict__ sorted) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.n_jobs) return;
  const uint2 pr = sorted[p];
  const uint64_t j = pr.y < a.n_jobs ? pr.y : 0;  // always the former; no index leaves the caller's arrays
  a.goff[p] = a.job_off[j];
  a.glen[p] = a.job_len[j];
  if (p == a.n_jobs - 1 && (uint64_t)pr.x >= a.n_streams) atomicOr(a.err, kErrStreamRow);
}

__global__ __launch_bounds__(256) void k_sjobs_begin(StreamJobsArgs a, const uint2* __restrict__ sorted) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t > a.n_streams) return;
  a.begin[t] = sj::lower_bound(a.n_jobs, t, [sorted](uint64_t p) { return sorted[p].x; });
}

unsigned grid256(uint64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

hipError_t launch_stream_jobs(const StreamJobsArgs& a, hipStream_t st, uint32_t* sort_launches,
                              uint32_t* row_launches) {
  *sort_launches = *row_launches = 0;
  if (a.n_jobs == 0 || a.n_jobs >= sj::kMaxJobs) return hipErrorInvalidValue;
  const dim3 tiles((unsigned)sj::tile_count(a.n_jobs)), wg(sj::kThreads);
  const uint64_t n_tiles = tiles.x;
  const dim3 digits(sj::kDigits), scan_wg(sj::kScanThreads);
  const uint2* in = nullptr;
  for (uint32_t pass = 0; pass < a.passes; ++pass) {
    uint2* out = a.pairs[sj::pass_output(pass)];
    if (pass == 0) {
      hipLaunchKernelGGL(k_sjobs_hist<true>, tiles, wg, 0, st, a, in, pass);
      hipLaunchKernelGGL(k_sjobs_scan, digits, scan_wg, 0, st, a.counts, n_tiles);
      hipLaunchKernelGGL(k_sjobs_scatter<true>, tiles, wg, 0, st, a, in, out, pass);
    } else {
      hipLaunchKernelGGL(k_sjobs_hist<false>, tiles, wg, 0, st, a, in, pass);
      hipLaunchKernelGGL(k_sjobs_scan, digits, scan_wg, 0, st, a.counts, n_tiles);
      hipLaunchKernelGGL(k_sjobs_scatter<false>, tiles, wg, 0, st, a, in, out, pass);
    }
    *sort_launches += 3;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    in = out;
  }
  hipLaunchKernelGGL(k_sjobs_rows, dim3(grid256(a.n_jobs)), dim3(256), 0, st, a, in);
  hipLaunchKernelGGL(k_sjobs_begin, dim3(grid256(a.n_streams + 1)), dim3(256), 0, st, a, in);
  *row_launches = 2;
  return hipGetLastError();
}

}  // namespace msha
