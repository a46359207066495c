// Device stream sets (gfx950 only): msha_dstreams_* (include/mirsha.h "Device stream
// sets"; DESIGN.md "Device stream sets").
//
// The host stream sets (streams.cpp, stream_kernels.hip) keep each stream's partial
// block and byte count on the host, so every write stages through pinned memory and
// waits. Here a stream is three rows of device memory -- eight state words, a 64-byte
// tail (bytes past length % 64 always zero) and a 64-bit length -- and Write, Sum, Snap
// and Reset are one kernel each with one lane per row, on the caller's stream.
//
// k_dstream_write gathers a row's parts with parts::fill_block (parts_gather.hpp, as
// k_digest_parts does, the block under assembly in an LDS slot of the lane's own 17
// dwords from the next: parts_kernels.hip tells why), the stream's buffered bytes in
// front of them as a virtual part served from the tail row (stream_device.hpp). Every
// read of the old tail row happens inside the first fill_block; the row is stored
// after the last one. No lane reads another's slot or another stream's rows: there is
// no barrier and no wave waits on another.
//
// Global accesses are 16 bytes a lane wherever a row allows it: the state as two, the
// tail row as four (rows are 64-byte aligned), an arena granule as one.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "parts_digest.hpp"
#include "stream_device.hpp"

namespace msha {

namespace {

__device__ __forceinline__ void row_load_state(const uint32_t* q, State& s) {
  const uint4 lo = reinterpret_cast<const uint4*>(q)[0];
  const uint4 hi = reinterpret_cast<const uint4*>(q)[1];
  s.h[0] = lo.x; s.h[1] = lo.y; s.h[2] = lo.z; s.h[3] = lo.w;
  s.h[4] = hi.x; s.h[5] = hi.y; s.h[6] = hi.z; s.h[7] = hi.w;
}
__device__ __forceinline__ void row_store_state(const State& s, uint32_t* q) {
  reinterpret_cast<uint4*>(q)[0] = make_uint4(s.h[0], s.h[1], s.h[2], s.h[3]);
  reinterpret_cast<uint4*>(q)[1] = make_uint4(s.h[4], s.h[5], s.h[6], s.h[7]);
}
__device__ __forceinline__ void row_store_tail(const uint32_t (&d)[16], uint8_t* trow) {
  uint4* q = reinterpret_cast<uint4*>(trow);
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = make_uint4(d[4 * i], d[4 * i + 1], d[4 * i + 2], d[4 * i + 3]);
}
// One 16-byte load, kept single (parts_digest.hpp: the compiler would split it by the
// dwords each byte phase selects).
__device__ __forceinline__ parts::Granule load_granule(const uint8_t* p) {
  uint4 v = *reinterpret_cast<const uint4*>(p);
  asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
  parts::Granule g;
  g.d[0] = v.x; g.d[1] = v.y; g.d[2] = v.z; g.d[3] = v.w;
  return g;
}
__device__ __forceinline__ void zero_digest(uint8_t* o) {
  reinterpret_cast<uint4*>(o)[0] = make_uint4(0, 0, 0, 0);
  reinterpret_cast<uint4*>(o)[1] = make_uint4(0, 0, 0, 0);
}

}  // namespace

__global__ __launch_bounds__(256, 8) void k_dstream_write(uint32_t* state, uint8_t* tail, uint64_t* length,
                                                         uint64_t n_streams, const uint8_t* __restrict__ arena,
                                                         const uint64_t* __restrict__ part_off,
                                                         const uint64_t* __restrict__ part_len,
                                                         const uint64_t* __restrict__ begin,
                                                         const uint32_t* __restrict__ row, uint64_t n_rows,
                                                         uint32_t* __restrict__ err) {
  __shared__ uint32_t slots[256 * kPartsSlotStride];
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  const uint64_t s = row ? (uint64_t)row[i] : i;
  if (s >= n_streams) {  // flagged; no stream is touched
    atomicOr(err, kErrStreamRow);
    return;
  }
  const uint64_t j0 = begin[i], jend = begin[i + 1];
  if (!dstream::range_ok(j0, jend)) {  // flagged; the stream stays as it was
    atomicOr(err, kErrPartsBegin);
    return;
  }
  if (jend == j0) return;  // nothing to append

  const uint64_t len = length[s];
  uint8_t* trow = tail + 64 * s;
  State st;
  row_load_state(state + 8 * s, st);

  uint32_t* slot = slots + threadIdx.x * kPartsSlotStride;
  auto slot_write = [slot](uint32_t j, uint32_t v) { slot[j] = v; };
  auto load = [arena, trow](uint64_t off) { return load_granule(dstream::tagged_address(off, arena, trow)); };
  auto block = [&st, slot]() {
    uint32_t raw[16], w[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) raw[j] = slot[j];
    to_words(raw, w);
    compress(st, w);
  };
  const dstream::Written wr =
      dstream::write_row((uint32_t)len & 63u, j0, (uint32_t)(jend - j0), part_off, part_len, slot_write, load, block);
  if (wr.appended == 0) return;  // empty parts only: nothing is stored

  uint32_t d[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) d[j] = dstream::tail_dword(slot[j], (uint32_t)j, wr.tail);
  row_store_tail(d, trow);
  if (wr.blocks != 0) row_store_state(st, state + 8 * s);
  length[s] = len + wr.appended;
}

// Sum: the digest of row i's stream to out + 32 i. SNAP: the stream then restarts as
// New() followed by Write(that digest) (recorder.go:298-300).
template <bool SNAP>
__global__ __launch_bounds__(256, 8) void k_dstream_finish(uint32_t* state, uint8_t* tail, uint64_t* length,
                                                          uint64_t n_streams, const uint32_t* __restrict__ row,
                                                          uint64_t n_rows, uint8_t* __restrict__ out,
                                                          uint32_t* __restrict__ err) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  const uint64_t s = row ? (uint64_t)row[i] : i;
  uint8_t* o = out + 32 * i;
  if (s >= n_streams) {  // flagged and zeroed, never a wrong digest
    atomicOr(err, kErrStreamRow);
    zero_digest(o);
    return;
  }
  const uint64_t len = length[s];
  const uint32_t t = (uint32_t)len & 63u;
  State st;
  row_load_state(state + 8 * s, st);
  uint32_t raw[16];
  load_block16(tail + 64 * s, raw);
  // the padded tail block, then the length block after a tail of 56 bytes or more: one
  // compress() call site, as in parts_digest.hpp
  for (int phase = 0; phase != 2;) {
    uint32_t w[16];
    if (phase == 0) {
      phase = build_tail(raw, t, len, w) ? 1 : 2;
    } else {
      length_block(len, w);
      phase = 2;
    }
    compress(st, w);
  }
  store_digest(st, o);
  if (SNAP) {
    uint32_t d[16];
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = bswap(st.h[j]);  // the digest's bytes as little-endian dwords
#pragma unroll
    for (int j = 8; j < 16; ++j) d[j] = 0;
    row_store_tail(d, tail + 64 * s);
    State iv;
    state_init(iv);
    row_store_state(iv, state + 8 * s);
    length[s] = 32;
  }
}

// Reset, and a new set's first state: the rows' streams are New().
__global__ __launch_bounds__(256) void k_dstream_reset(uint32_t* state, uint8_t* tail, uint64_t* length,
                                                      uint64_t n_streams, const uint32_t* __restrict__ row,
                                                      uint64_t n_rows, uint32_t* __restrict__ err) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  const uint64_t s = row ? (uint64_t)row[i] : i;
  if (s >= n_streams) {
    atomicOr(err, kErrStreamRow);
    return;
  }
  uint32_t d[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) d[j] = 0;
  row_store_tail(d, tail + 64 * s);
  State iv;
  state_init(iv);
  row_store_state(iv, state + 8 * s);
  length[s] = 0;
}

// Whole streams to and from packed rows of dstream::kRowDwords dwords (export, import;
// the host has checked the ids). packed[i] <-> stream id ? id[i] : i.
__global__ __launch_bounds__(256) void k_dstream_rows_get(const uint32_t* __restrict__ state,
                                                         const uint8_t* __restrict__ tail,
                                                         const uint64_t* __restrict__ length,
                                                         const uint32_t* __restrict__ id, uint64_t k,
                                                         uint32_t* __restrict__ packed) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const uint64_t s = id ? (uint64_t)id[i] : i;
  uint32_t* p = packed + dstream::kRowDwords * i;
  const uint32_t* t = reinterpret_cast<const uint32_t*>(tail + 64 * s);
  for (int j = 0; j < 8; ++j) p[j] = state[8 * s + j];
  for (int j = 0; j < 16; ++j) p[8 + j] = t[j];
  const uint64_t len = length[s];
  p[24] = (uint32_t)len;
  p[25] = (uint32_t)(len >> 32);
}

__global__ __launch_bounds__(256) void k_dstream_rows_set(uint32_t* __restrict__ state, uint8_t* __restrict__ tail,
                                                         uint64_t* __restrict__ length,
                                                         const uint32_t* __restrict__ id, uint64_t k,
                                                         const uint32_t* __restrict__ packed) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const uint64_t s = id ? (uint64_t)id[i] : i;
  const uint32_t* p = packed + dstream::kRowDwords * i;
  uint32_t* t = reinterpret_cast<uint32_t*>(tail + 64 * s);
  for (int j = 0; j < 8; ++j) state[8 * s + j] = p[j];
  for (int j = 0; j < 16; ++j) t[j] = p[8 + j];
  length[s] = (uint64_t)p[25] << 32 | p[24];
}

static inline dim3 dstream_grid(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }

hipError_t launch_dstream_write(const DstreamRows& r, const uint8_t* arena, const uint64_t* part_off,
                                const uint64_t* part_len, const uint64_t* begin, const uint32_t* row,
                                uint64_t n_rows, uint32_t* err, hipStream_t st) {
  if (n_rows == 0) return hipSuccess;
  hipLaunchKernelGGL(k_dstream_write, dstream_grid(n_rows), dim3(256), 0, st, r.state, r.tail, r.length, r.n, arena,
                     part_off, part_len, begin, row, n_rows, err);
  return hipGetLastError();
}

hipError_t launch_dstream_finish(const DstreamRows& r, const uint32_t* row, uint64_t n_rows, uint8_t* out, bool snap,
                                 uint32_t* err, hipStream_t st) {
  if (n_rows == 0) return hipSuccess;
  if (snap)
    hipLaunchKernelGGL(k_dstream_finish<true>, dstream_grid(n_rows), dim3(256), 0, st, r.state, r.tail, r.length,
                       r.n, row, n_rows, out, err);
  else
    hipLaunchKernelGGL(k_dstream_finish<false>, dstream_grid(n_rows), dim3(256), 0, st, r.state, r.tail, r.length,
                       r.n, row, n_rows, out, err);
  return hipGetLastError();
}

hipError_t launch_dstream_reset(const DstreamRows& r, const uint32_t* row, uint64_t n_rows, uint32_t* err,
                                hipStream_t st) {
  if (n_rows == 0) return hipSuccess;
  hipLaunchKernelGGL(k_dstream_reset, dstream_grid(n_rows), dim3(256), 0, st, r.state, r.tail, r.length, r.n, row,
                     n_rows, err);
  return hipGetLastError();
}

hipError_t launch_dstream_rows_get(const DstreamRows& r, const uint32_t* id, uint64_t k, uint32_t* packed,
                                   hipStream_t st) {
  if (k == 0) return hipSuccess;
  hipLaunchKernelGGL(k_dstream_rows_get, dstream_grid(k), dim3(256), 0, st, r.state, r.tail, r.length, id, k, packed);
  return hipGetLastError();
}

hipError_t launch_dstream_rows_set(const DstreamRows& r, const uint32_t* id, uint64_t k, const uint32_t* packed,
                                   hipStream_t st) {
  if (k == 0) return hipSuccess;
  hipLaunchKernelGGL(k_dstream_rows_set, dstream_grid(k), dim3(256), 0, st, r.state, r.tail, r.length, id, k, packed);
  return hipGetLastError();
}

}  // namespace msha
