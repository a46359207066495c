// One lane's work in k_dstream_write_rest (stream_chain.hip, device only): row i's
// parts appended to its stream -- the gather of stream_device.hpp, the compressions, the
// tail row and the length stored. It is k_dstream_write's row body (stream_device.hip),
// statement for statement; everything that decides a byte is in stream_device.hpp, which
// both use. k_dstream_write keeps its own text: calling this function from it gave that
// kernel another register allocation, and its code is to stay as it is
// (profiles/streams_device/README.md records the comparison).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sha256_device.hpp"
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

}  // namespace

// slots: the workgroup's 256 x kPartsSlotStride dwords of LDS. i < n_rows.
__device__ __forceinline__ void dstream_write_lane(uint32_t* state, uint8_t* tail, uint64_t* length,
                                                   uint64_t n_streams, const uint8_t* arena,
                                                   const uint64_t* part_off,
                                                   const uint64_t* part_len,
                                                   const uint64_t* begin,
                                                   const uint32_t* row, uint64_t i,
                                                   uint32_t* err, uint32_t* slots) {
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

}  // namespace msha
