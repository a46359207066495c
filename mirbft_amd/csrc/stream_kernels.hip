// Resume kernels of the stream sets (gfx950 only): SHA-256 continued from a
// chaining state instead of the IV, and padded for a total length that includes
// the bytes hashed before.
//
// They serve the streaming half of processor.Hasher, New() hash.Hash
// (pkg/processor/serial.go:21-23): Write appends, Sum(b) appends
// the digest without resetting -- the way NodeState.Apply / Snap use it
// (pkg/testengine/recorder.go:288-359). One stream is one lane, as
// one message is in kernels.hip; the host (streams.cpp) keeps each stream's
// partial block and byte count, so these kernels only ever see whole blocks
// (absorb) or a message's last bytes together with its total length (finish).
// No wave waits on another here: no flags, no hand-offs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "sha256_device.hpp"
#include "kernels.hpp"

namespace msha {

// Blocks of one lane, from state s. FINAL == false: `work` whole blocks at p, no
// padding. FINAL == true: the last `work` bytes of a message of prefix + work
// bytes: its whole blocks, the tail block (build_tail masks every byte at or
// past the end) and, for a tail of 56 bytes or more, the length block. The loop
// is hash_message's (kernels.hip): one compress() call site, the same three load
// modes, blocks read 64 bytes at a time (the block after a lane's last whole one
// is read too: the arena's slack keeps that in bounds). The wave-uniform padding
// path (compress_uniform_pad) is left out.
template <int MODE, bool FINAL>
__device__ __forceinline__ void stream_blocks(State& s, const uint8_t* p, uint64_t work, uint64_t prefix) {
  const uint32_t nfull = FINAL ? (uint32_t)(work >> 6) : (uint32_t)work;  // < 2^32 blocks
  const uint32_t r = FINAL ? (uint32_t)(work & 63) : 0u;
  const uint32_t nblocks = FINAL ? nfull + (r < 56 ? 1 : 2) : nfull;
  const uint64_t total = prefix + work;  // FINAL: the message's length in bytes
  uint32_t raw[16];
  uint32_t w[16];
  constexpr int LM = MODE;
  if (LM == kPrefetch) load_block16<MODE>(p, raw);
  for (uint32_t b = 0; b < nblocks; ++b) {
    const uint8_t* pb = p + 64 * (uint64_t)b;
    if (LM == kSingle && b <= nfull) load_block16<MODE>(pb, raw);
    if (LM == kPair && b == nfull && !(b & 1)) load_block16<MODE>(pb, raw);
    if (b < nfull) {
      if (LM == kPair) {
        if (!(b & 1)) {
          uint32_t t[16];
          load_block16<MODE>(pb, t);
          load_block16<MODE>(pb + 64, raw);  // block b+1, or the bytes after the last block (slack-safe)
          to_words(t, w);
        } else {
          to_words(raw, w);
        }
      } else {
        to_words(raw, w);
        if (LM == kPrefetch) load_block16<MODE>(pb + 64, raw);
      }
    } else if (b == nfull) {  // FINAL only (nblocks == nfull otherwise)
      uint32_t rr = r;
      asm volatile("" : "+v"(rr));  // the tail masks built here, not hoisted (kernels.hip hash_message)
      build_tail(raw, rr, total, w);
    } else {
      length_block(total, w);
    }
    compress(s, w);
  }
}

__device__ __forceinline__ void load_state(const uint32_t* q, State& s) {
  const uint4 lo = reinterpret_cast<const uint4*>(q)[0];
  const uint4 hi = reinterpret_cast<const uint4*>(q)[1];
  s.h[0] = lo.x; s.h[1] = lo.y; s.h[2] = lo.z; s.h[3] = lo.w;
  s.h[4] = hi.x; s.h[5] = hi.y; s.h[6] = hi.z; s.h[7] = hi.w;
}
__device__ __forceinline__ void store_state(const State& s, uint32_t* q) {
  reinterpret_cast<uint4*>(q)[0] = make_uint4(s.h[0], s.h[1], s.h[2], s.h[3]);
  reinterpret_cast<uint4*>(q)[1] = make_uint4(s.h[4], s.h[5], s.h[6], s.h[7]);
}

template <int MODE>
__global__ __launch_bounds__(256, 8) void k_stream_absorb(uint32_t* __restrict__ state,
                                                       const uint8_t* __restrict__ arena,
                                                       const uint64_t* __restrict__ off,
                                                       const uint64_t* __restrict__ nblocks,
                                                       const uint32_t* __restrict__ row, uint64_t n,
                                                       uint32_t* __restrict__ err) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t nb = nblocks[i];
  if (nb == 0) return;
  const uint8_t* p = arena + off[i];
  if ((reinterpret_cast<uintptr_t>(p) & 15) != 0) {  // flagged; the state stays as it was
    atomicOr(err, 1u);
    return;
  }
  uint32_t* q = state + 8 * (row ? (uint64_t)row[i] : i);
  State s;
  load_state(q, s);
  stream_blocks<MODE, false>(s, p, nb, 0);
  store_state(s, q);
}

template <int MODE>
__global__ __launch_bounds__(256, 8) void k_stream_finish(const uint32_t* __restrict__ state,
                                                       const uint64_t* __restrict__ prefix,
                                                       const uint8_t* __restrict__ arena,
                                                       const uint64_t* __restrict__ off,
                                                       const uint64_t* __restrict__ len,
                                                       const uint32_t* __restrict__ row, uint64_t n,
                                                       uint8_t* __restrict__ out, uint32_t* __restrict__ err) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t* p = arena + off[i];
  uint8_t* o = out + 32 * i;
  if ((reinterpret_cast<uintptr_t>(p) & 15) != 0) {  // flagged and zeroed, never a wrong digest
    atomicOr(err, 1u);
    reinterpret_cast<uint4*>(o)[0] = make_uint4(0, 0, 0, 0);
    reinterpret_cast<uint4*>(o)[1] = make_uint4(0, 0, 0, 0);
    return;
  }
  State s;
  if (state) load_state(state + 8 * (row ? (uint64_t)row[i] : i), s);
  else state_init(s);
  stream_blocks<MODE, true>(s, p, len[i], prefix ? prefix[i] : 0);
  store_digest(s, o);
}

// state[row[i]] = vals[i], or the IV (reset, import)
__global__ __launch_bounds__(256) void k_stream_rows_set(uint32_t* __restrict__ state,
                                                        const uint32_t* __restrict__ row,
                                                        const uint32_t* __restrict__ vals, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  State s;
  if (vals) load_state(vals + 8 * i, s);
  else state_init(s);
  store_state(s, state + 8 * (row ? (uint64_t)row[i] : i));
}

// out[i] = state[row[i]] (export)
__global__ __launch_bounds__(256) void k_stream_rows_get(const uint32_t* __restrict__ state,
                                                        const uint32_t* __restrict__ row,
                                                        uint32_t* __restrict__ out, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  State s;
  load_state(state + 8 * (row ? (uint64_t)row[i] : i), s);
  store_state(s, out + 8 * i);
}

static inline unsigned stream_grid(uint64_t n) { return (unsigned)((n + 255) / 256); }

// pick_mode's choice for the launch; its kPipe range (at most a wave per SIMD) runs
// the prefetching variant.
static inline int stream_mode(uint64_t n, int cus, int* mode) {
  int m = pick_mode(n, cus);
  if (m == kPipe) m = kPrefetch;
  if (mode) *mode = m;
  return m;
}

template <class F>
static inline void with_stream_mode(int mode, F&& f) {
  switch (mode) {
    case kSingle: f(std::integral_constant<int, kSingle>()); break;
    case kPrefetch: f(std::integral_constant<int, kPrefetch>()); break;
    default: f(std::integral_constant<int, kPair>()); break;
  }
}

hipError_t launch_stream_absorb(uint32_t* state, const uint8_t* arena, const uint64_t* off,
                                const uint64_t* nblocks, const uint32_t* row, uint64_t n, uint32_t* err,
                                int cus, hipStream_t st, int* mode) {
  if (n == 0) return hipSuccess;
  with_stream_mode(stream_mode(n, cus, mode), [&](auto m) {
    hipLaunchKernelGGL(k_stream_absorb<decltype(m)::value>, dim3(stream_grid(n)), dim3(256), 0, st, state,
                       arena, off, nblocks, row, n, err);
  });
  return hipGetLastError();
}

hipError_t launch_stream_finish(const uint32_t* state, const uint64_t* prefix, const uint8_t* arena,
                                const uint64_t* off, const uint64_t* len, const uint32_t* row, uint64_t n,
                                uint8_t* out, uint32_t* err, int cus, hipStream_t st, int* mode) {
  if (n == 0) return hipSuccess;
  with_stream_mode(stream_mode(n, cus, mode), [&](auto m) {
    hipLaunchKernelGGL(k_stream_finish<decltype(m)::value>, dim3(stream_grid(n)), dim3(256), 0, st, state,
                       prefix, arena, off, len, row, n, out, err);
  });
  return hipGetLastError();
}

hipError_t launch_stream_rows_set(uint32_t* state, const uint32_t* row, const uint32_t* vals, uint64_t n,
                                  hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_stream_rows_set, dim3(stream_grid(n)), dim3(256), 0, st, state, row, vals, n);
  return hipGetLastError();
}

hipError_t launch_stream_rows_get(const uint32_t* state, const uint32_t* row, uint32_t* out, uint64_t n,
                                  hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_stream_rows_get, dim3(stream_grid(n)), dim3(256), 0, st, state, row, out, n);
  return hipGetLastError();
}

}  // namespace msha
