// msha_concat_lists_device (gfx950 only): part lists flattened into contiguous, 16-byte
// aligned messages, the form every chain kernel here wants (include/mirsha.h "Part
// lists flattened on the GPU").
//
// Three kernels on the caller's stream, no workspace, no memset, no host wait:
//   k_concat_measure  per message: is its list valid, and the sum of its part lengths
//                     (msg_len[k]; msg_off[k] = 1 marks an invalid one until the scan).
//                     k_parts_measure's rule: a lane sums a short list, the wave a list
//                     of wave_sum_parts parts or more with coalesced part_len loads.
//   k_concat_scan     ONE workgroup walks the messages kScanWidth at a time with a
//                     carry: lengths -> offsets (a running sum of round16(len)), the fit
//                     rule, off = len = 0 for what is refused, the error bit. Nothing
//                     waits for another workgroup, so nothing can spin.
//   k_concat_copy     a workgroup per message; placement in parts_concat.hpp. A step
//                     takes kStepParts parts, a thread each: (off, len) loaded, a block
//                     scan of len (wave shuffles, the wave totals in LDS) -> positions.
//                     The step's bytes reach dst through an LDS image a window at a
//                     time: parts below kLargePart bytes are copied by their own
//                     thread, larger ones by all 256 a source granule each; then the
//                     image's complete granules are stored as coalesced 16-byte
//                     vectors and the rest carries to the next window. Only the
//                     workgroup that owns a message writes its granules: no atomics on
//                     dst, and no byte outside [off, off + round16(len)) is written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mirsha.h"
#include "kernels.hpp"
#include "parts_concat.hpp"

namespace msha {

namespace {

namespace pc = parts_concat;

__device__ __forceinline__ uint32_t wave_lane() { return threadIdx.x & 63u; }

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor((unsigned long long)v, d);
  return v;
}

// Inclusive scan over the wave.
__device__ __forceinline__ uint64_t wave_scan(uint64_t v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t up = __shfl_up((unsigned long long)v, d);
    if ((int)wave_lane() >= d) v += up;
  }
  return v;
}

__global__ __launch_bounds__(256) void k_concat_measure(ConcatArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool lane = k < a.n_select;
  uint64_t j0 = 0, np = 0;
  bool bad = false;
  if (lane) {
    const uint64_t s = a.select ? (uint64_t)a.select[k] : k;
    bad = s >= a.n_lists;
    if (!bad) {
      j0 = a.begin[s];
      const uint64_t jend = a.begin[s + 1];
      bad = jend < j0 || jend - j0 > 0xffffffffull;
      np = bad ? 0 : jend - j0;
    }
  }
  const bool wide = lane && np >= a.wave_sum_parts;
  uint64_t total = 0;
  if (lane && !wide)
    for (uint64_t j = 0; j < np; ++j) total += a.part_len[j0 + j];
  // the long lists of this wave, one after the other, by all 64 lanes
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
  if (lane) {
    a.msg_len[k] = total;
    a.msg_off[k] = bad ? 1 : 0;
  }
}

__global__ __launch_bounds__(pc::kScanThreads) void k_concat_scan(ConcatArgs a) {
  __shared__ uint64_t wsum[pc::kScanThreads / 64];
  uint64_t carry = 0;
  bool refused = false;
  for (uint64_t k0 = 0; k0 < a.n_select; k0 += pc::kScanWidth) {
    const uint64_t k = k0 + (uint64_t)threadIdx.x * pc::kScanPer;
    uint64_t len[pc::kScanPer], r[pc::kScanPer], s = 0;
    bool bad[pc::kScanPer];
#pragma unroll
    for (uint32_t j = 0; j < pc::kScanPer; ++j) {
      const bool in = k + j < a.n_select;
      len[j] = in ? a.msg_len[k + j] : 0;
      bad[j] = in && a.msg_off[k + j] != 0;
      r[j] = bad[j] ? 0 : pc::round16(len[j]);  // an invalid list counts as length 0
      s += r[j];
    }
    const uint64_t inc = wave_scan(s);
    if (wave_lane() == 63) wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint64_t base = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < pc::kScanThreads / 64; ++w) {
      if (w < (threadIdx.x >> 6)) base += wsum[w];
      all += wsum[w];
    }
    uint64_t start = carry + base + inc - s;
#pragma unroll
    for (uint32_t j = 0; j < pc::kScanPer; ++j) {
      if (k + j < a.n_select) {
        const bool ok = !bad[j] && pc::fits(start, len[j], a.dst_bytes, MSHA_DEVICE_ARENA_SLACK);
        a.msg_off[k + j] = ok ? start : 0;
        if (!ok) {
          a.msg_len[k + j] = 0;
          refused = true;
        }
      }
      start += r[j];
    }
    carry += all;
    __syncthreads();  // wsum is written again
  }
  if (refused) atomicOr(a.err, kErrPartsConcat);
}

__global__ __launch_bounds__(256) void k_concat_copy(ConcatArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t img[pc::kImageBytes / 4];
  __shared__ uint64_t s_off[pc::kStepParts], s_len[pc::kStepParts], s_pos[pc::kStepParts];
  __shared__ uint64_t s_wsum[pc::kStepParts / 64];
  __shared__ uint32_t s_large[pc::kStepParts];
  __shared__ uint32_t s_nlarge;
  static_assert(pc::kStepParts == 256, "a step is one part a thread of a 256-thread workgroup");
  uint8_t* const img8 = reinterpret_cast<uint8_t*>(img);
  const uint4* const img16 = reinterpret_cast<const uint4*>(img);
  const uint32_t t = threadIdx.x;

  const uint8_t* const arena = a.arena;
  auto load = [&](uint64_t off) {
    const uint4 v = *reinterpret_cast<const uint4*>(arena + off);
    parts::Granule g;
    g.d[0] = v.x;
    g.d[1] = v.y;
    g.d[2] = v.z;
    g.d[3] = v.w;
    return g;
  };
  auto st32 = [&](uint32_t d, uint32_t v) { img[d] = v; };
  auto st8 = [&](uint32_t x, uint32_t v) { img8[x] = (uint8_t)v; };

  for (uint64_t k = blockIdx.x; k < a.n_select; k += gridDim.x) {
    const uint64_t total = a.msg_len[k];  // 0 as well for a refused message: nothing of its list is read
    if (total == 0) continue;             // the same for every thread of the workgroup
    const uint64_t s = a.select ? (uint64_t)a.select[k] : k;
    const uint64_t j0 = a.begin[s], np = a.begin[s + 1] - j0;
    uint4* const dst = reinterpret_cast<uint4*>(a.dst + a.msg_off[k]);
    if (t == 0) s_nlarge = 0;
    uint64_t base = 0;  // message bytes placed by the steps before
    uint64_t noff = 0, nlen = 0;  // the next step's part of this thread, fetched a step ahead
    if (t < np) {
      noff = a.part_off[j0 + t];
      nlen = a.part_len[j0 + t];
    }
    for (uint64_t p0 = 0; p0 < np; p0 += pc::kStepParts) {
      const uint64_t off = noff, len = nlen;
      noff = nlen = 0;
      if (p0 + pc::kStepParts + t < np) {
        noff = a.part_off[j0 + p0 + pc::kStepParts + t];
        nlen = a.part_len[j0 + p0 + pc::kStepParts + t];
      }
      const uint64_t inc = wave_scan(len);
      if (wave_lane() == 63) s_wsum[t >> 6] = inc;
      __syncthreads();
      uint64_t wbase = 0, step = 0;
#pragma unroll
      for (uint32_t w = 0; w < pc::kStepParts / 64; ++w) {
        if (w < (t >> 6)) wbase += s_wsum[w];
        step += s_wsum[w];
      }
      const uint64_t pos = base + wbase + inc - len;
      const bool large = len >= pc::kLargePart;
      if (large) {
        const uint32_t i = atomicAdd(&s_nlarge, 1u);
        s_large[i] = t;
        s_off[t] = off;
        s_len[t] = len;
        s_pos[t] = pos;
      }
      __syncthreads();
      const uint32_t nlarge = s_nlarge;
      const uint64_t step_end = base + step;
      uint64_t cur = base;
      while (cur < step_end) {
        const pc::Window w = pc::window_at(cur, step_end);
        if (!large) {
          const pc::Piece pp = pc::clip(pos, len, w);
          if (pp.n) pc::copy_piece(off + pp.skip, pp.n, (uint32_t)(pos + pp.skip - w.wb), load, st32, st8);
        }
        for (uint32_t i = 0; i < nlarge; ++i) {
          const uint32_t l = s_large[i];
          const uint64_t lpos = s_pos[l];
          const pc::Piece pp = pc::clip(lpos, s_len[l], w);
          pc::coop_piece(s_off[l] + pp.skip, pp.n, (uint32_t)(lpos + pp.skip - w.wb), t, pc::kStepParts, load, st32,
                         st8);
        }
        __syncthreads();
        const uint32_t ng = pc::window_granules(w), rest = pc::window_rest(w);
        uint4* const out = dst + (w.wb >> 4);
        for (uint32_t g = t; g < ng; g += pc::kStepParts) out[g] = img16[g];
        const uint8_t cb = t < rest ? img8[16u * ng + t] : (uint8_t)0;
        __syncthreads();
        if (t < rest) img8[t] = cb;  // the carry; the next window writes from byte `rest` on
        cur = w.hi;
      }
      base = step_end;
      __syncthreads();  // every thread has read s_nlarge, s_large and s_wsum of this step
      if (t == 0) s_nlarge = 0;
    }
    const uint32_t r = (uint32_t)(base & 15u);
    if (r != 0 && t == 0) {
      const uint4 c = img16[0];
      uint32_t v[4] = {c.x, c.y, c.z, c.w};
      pc::last_granule(v, r);
      dst[base >> 4] = make_uint4(v[0], v[1], v[2], v[3]);
    }
    __syncthreads();  // the image and s_nlarge are the next message's
  }
}

unsigned grid256(uint64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

hipError_t launch_concat_measure(const ConcatArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_concat_measure, dim3(grid256(a.n_select)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_concat_scan(const ConcatArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_concat_scan, dim3(1), dim3(pc::kScanThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_concat_copy(const ConcatArgs& a, hipStream_t st) {
  // a workgroup per message, up to 2^22 workgroups (grid x block stays below 2^32); past
  // that a workgroup takes several messages
  const uint64_t cap = 1ull << 22;
  hipLaunchKernelGGL(k_concat_copy, dim3((unsigned)(a.n_select < cap ? a.n_select : cap)), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace msha
