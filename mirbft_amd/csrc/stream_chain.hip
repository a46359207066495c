// msha_dstreams_write_routed_device (gfx950 only): Write with its long rows on the
// eight-lane chain (include/mirsha.h "Device stream sets: long writes routed to the
// chain"). In a device stream set one stream is one lane, so a few streams
// that each take thousands of digests run at a handful of lanes' rate. Here the call
// finds such rows on the GPU and gives each eight lanes:
//   k_sroute_init     claim counters to 0, every slot unfilled, the row flags cleared
//   k_sroute_measure  per row: the stream's buffered bytes t, the sum of its part lengths
//                     (a lane sums a short list, the wave a long one, as k_concat_measure),
//                     the decision (stream_chain.hpp is_long_row), the claims
//                     (parts_route.hpp: a slot, then room), the slot's arrays, taken[r] = 1
//   k_sroute_copy     a workgroup per filled slot: the t buffered bytes, then the parts,
//                     back to back from a 16-aligned start with a zeroed pad. It is
//                     k_concat_copy's loop (placement: parts_concat.hpp) over one part
//                     more: part 0 is the tail row, named by the tagged offset kTailTag
//                     (stream_device.hpp), and the load callback reads a tagged offset
//                     from that row
//   k_absorb_chain8   (kernels.hip) over the slots: the stream's state row in, the
//                     message's whole blocks, the state row out
//   k_sroute_tail     per filled slot: what the message holds past its whole blocks is
//                     the stream's new tail row, zero past it; length += the parts' sum
//   k_dstream_write_rest  Write's row body (stream_write.hpp) over the rows not taken;
//                     invalid rows are flagged here and nowhere else
// No kernel waits on another workgroup; a routed row's stream is touched by the copy
// (read), the chain and the tail only, every other row's by the last kernel only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "parts_concat.hpp"
#include "stream_chain.hpp"
#include "stream_write.hpp"

namespace msha {

namespace {

namespace pc = parts_concat;
namespace pr = parts_route;

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

__global__ __launch_bounds__(256) void k_sroute_init(StreamRouteArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (a.n_rows + 3) / 4) reinterpret_cast<uint32_t*>(a.taken)[i] = 0;
  if (i < a.max_long) {
    a.slot_row[i] = 0;
    a.slot_stream[i] = schain::kNoStream;
    a.slot_t[i] = 0;
    a.msg_off[i] = 0;
    a.msg_len[i] = pr::kUnfilledLen;
    a.blocks[i] = 0;
  }
  if (i < pr::kClaimWords) a.claim[i] = 0;
}

__global__ __launch_bounds__(256) void k_sroute_measure(StreamRouteArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool valid = r < a.n_rows;
  uint64_t s = 0, j0 = 0, np = 0;
  if (valid) {
    s = a.row ? (uint64_t)a.row[r] : r;
    valid = s < a.rows.n;
  }
  if (valid) {
    j0 = a.begin[r];
    const uint64_t jend = a.begin[r + 1];
    valid = dstream::range_ok(j0, jend);
    np = valid ? jend - j0 : 0;
  }
  const bool wide = valid && np >= a.wave_sum_parts;
  uint64_t sum = 0;
  if (valid && !wide)
    for (uint64_t j = 0; j < np; ++j) sum += a.part_len[j0 + j];
  // the long lists of this wave, one after the other, by all 64 lanes
  uint64_t pending = __ballot(wide);
  while (pending) {
    const int lead = __ffsll((unsigned long long)pending) - 1;
    pending &= pending - 1;
    const uint64_t wj0 = __shfl((unsigned long long)j0, lead), wnp = __shfl((unsigned long long)np, lead);
    uint64_t x = 0;
    for (uint64_t j = wave_lane(); j < wnp; j += 64) x += a.part_len[wj0 + j];
    x = wave_sum(x);
    if ((int)wave_lane() == lead) sum = x;
  }
  if (!valid || np == 0) return;  // an invalid row is the last kernel's to flag
  const uint32_t t = (uint32_t)a.rows.length[s] & 63u;
  if (!schain::is_long_row(t, sum, a.long_blocks)) return;
  const uint64_t total = schain::message_len(t, sum);
  uint64_t next = 0;
  if (!pr::room_ok(0, total, a.long_bytes, kArenaSlack, &next)) return;  // it could never fit
  const uint64_t ticket = atomicAdd(&a.claim[pr::kClaimSlots], 1ull);
  if (!pr::slot_ok(ticket, a.max_long)) return;
  unsigned long long* const given = &a.claim[pr::kClaimBytes];
  uint64_t cur = __atomic_load_n(given, __ATOMIC_RELAXED);
  bool routed = false;
  while (pr::room_ok(cur, total, a.long_bytes, kArenaSlack, &next)) {
    const uint64_t seen = atomicCAS(given, (unsigned long long)cur, (unsigned long long)next);
    if (seen == cur) {
      routed = true;
      break;
    }
    cur = seen;
  }
  if (!routed) return;  // the slot stays unfilled
  const uint32_t k = (uint32_t)ticket;
  a.slot_row[k] = (uint32_t)r;
  a.slot_stream[k] = (uint32_t)s;
  a.slot_t[k] = t;
  a.msg_off[k] = cur;
  a.msg_len[k] = total;
  a.blocks[k] = schain::whole_blocks(t, sum);
  a.taken[r] = 1;
  atomicAdd(&a.claim[pr::kClaimRouted], 1ull);
}

__global__ __launch_bounds__(256) void k_sroute_copy(StreamRouteArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t img[pc::kImageBytes / 4];
  __shared__ uint64_t s_off[pc::kStepParts], s_len[pc::kStepParts], s_pos[pc::kStepParts];
  __shared__ uint64_t s_wsum[pc::kStepParts / 64];
  __shared__ uint32_t s_large[pc::kStepParts];
  __shared__ uint32_t s_nlarge;
  static_assert(pc::kStepParts == 256, "a step is one part a thread of a 256-thread workgroup");
  uint8_t* const img8 = reinterpret_cast<uint8_t*>(img);
  const uint4* const img16 = reinterpret_cast<const uint4*>(img);
  const uint32_t t = threadIdx.x;
  auto st32 = [&](uint32_t d, uint32_t v) { img[d] = v; };
  auto st8 = [&](uint32_t x, uint32_t v) { img8[x] = (uint8_t)v; };

  for (uint64_t k = blockIdx.x; k < a.max_long; k += gridDim.x) {
    const uint64_t total = a.msg_len[k];  // 0 for an unfilled slot
    if (total == 0) continue;             // the same for every thread of the workgroup
    const uint64_t r = a.slot_row[k];
    const uint8_t* const arena = a.arena;
    const uint8_t* const trow = a.rows.tail + 64 * (uint64_t)a.slot_stream[k];
    const uint64_t buffered = a.slot_t[k];
    auto load = [arena, trow](uint64_t off) {
      const uint4 v = *reinterpret_cast<const uint4*>(dstream::tagged_address(off, arena, trow));
      parts::Granule g;
      g.d[0] = v.x;
      g.d[1] = v.y;
      g.d[2] = v.z;
      g.d[3] = v.w;
      return g;
    };
    // part q of the message: the tail row's bytes for q == 0, the row's part q - 1 after it
    const uint64_t j0 = a.begin[r], np = a.begin[r + 1] - j0 + 1;
    auto part = [&](uint64_t q, uint64_t& off, uint64_t& len) {
      off = q == 0 ? dstream::kTailTag : a.part_off[j0 + q - 1];
      len = q == 0 ? buffered : a.part_len[j0 + q - 1];
    };
    uint4* const dst = reinterpret_cast<uint4*>(a.flat + a.msg_off[k]);
    if (t == 0) s_nlarge = 0;
    uint64_t base = 0;  // message bytes placed by the steps before
    uint64_t noff = 0, nlen = 0;  // the next step's part of this thread, fetched a step ahead
    if (t < np) part(t, noff, nlen);
    for (uint64_t p0 = 0; p0 < np; p0 += pc::kStepParts) {
      const uint64_t off = noff, len = nlen;
      noff = nlen = 0;
      if (p0 + pc::kStepParts + t < np) part(p0 + pc::kStepParts + t, noff, nlen);
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
      const bool large = len >= pc::kLargePart;  // never the tail row: it holds fewer than 64 bytes
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
    const uint32_t rem = (uint32_t)(base & 15u);
    if (rem != 0 && t == 0) {
      const uint4 c = img16[0];
      uint32_t v[4] = {c.x, c.y, c.z, c.w};
      pc::last_granule(v, rem);
      dst[base >> 4] = make_uint4(v[0], v[1], v[2], v[3]);
    }
    __syncthreads();  // the image and s_nlarge are the next slot's
  }
}

__global__ __launch_bounds__(256) void k_sroute_tail(StreamRouteArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= a.max_long) return;
  const uint32_t s = a.slot_stream[k];
  if (s == schain::kNoStream) return;
  const uint64_t total = a.msg_len[k], whole = a.blocks[k];
  const uint32_t rem = schain::tail_bytes(total, whole);
  const uint4* const src = reinterpret_cast<const uint4*>(a.flat + a.msg_off[k] + 64 * whole);
  uint32_t d[16];
#pragma unroll
  for (uint32_t g = 0; g < 4; ++g) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (schain::tail_granule_read(g, rem)) v = src[g];
    d[4 * g] = schain::tail_row_dword(v.x, 4 * g, rem);
    d[4 * g + 1] = schain::tail_row_dword(v.y, 4 * g + 1, rem);
    d[4 * g + 2] = schain::tail_row_dword(v.z, 4 * g + 2, rem);
    d[4 * g + 3] = schain::tail_row_dword(v.w, 4 * g + 3, rem);
  }
  row_store_tail(d, a.rows.tail + 64 * (uint64_t)s);
  a.rows.length[s] = schain::new_length(a.rows.length[s], total - a.slot_t[k]);
}

__global__ __launch_bounds__(256, 8) void k_dstream_write_rest(uint32_t* state, uint8_t* tail, uint64_t* length,
                                                              uint64_t n_streams, const uint8_t* __restrict__ arena,
                                                              const uint64_t* __restrict__ part_off,
                                                              const uint64_t* __restrict__ part_len,
                                                              const uint64_t* __restrict__ begin,
                                                              const uint32_t* __restrict__ row, uint64_t n_rows,
                                                              const uint8_t* __restrict__ taken,
                                                              uint32_t* __restrict__ err) {
  __shared__ uint32_t slots[256 * kPartsSlotStride];
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  if (taken[i] != 0) return;  // the chain's
  dstream_write_lane(state, tail, length, n_streams, arena, part_off, part_len, begin, row, i, err, slots);
}

unsigned grid256(uint64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

hipError_t launch_sroute_init(const StreamRouteArgs& a, hipStream_t st) {
  uint64_t words = (a.n_rows + 3) / 4;
  if (a.max_long > words) words = a.max_long;
  if (pr::kClaimWords > words) words = pr::kClaimWords;
  hipLaunchKernelGGL(k_sroute_init, dim3(grid256(words)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_sroute_measure(const StreamRouteArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_sroute_measure, dim3(grid256(a.n_rows)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_sroute_copy(const StreamRouteArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_sroute_copy, dim3(a.max_long), dim3(256), 0, st, a);  // max_long <= 16 x CUs
  return hipGetLastError();
}

hipError_t launch_sroute_tail(const StreamRouteArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_sroute_tail, dim3(grid256(a.max_long)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_dstream_write_rest(const StreamRouteArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_dstream_write_rest, dim3(grid256(a.n_rows)), dim3(256), 0, st, a.rows.state, a.rows.tail,
                     a.rows.length, a.rows.n, a.arena, a.part_off, a.part_len, a.begin, a.row, a.n_rows, a.taken,
                     a.err);
  return hipGetLastError();
}

}  // namespace msha
