// One lane's work in the parts kernels (device only): action a's parts gathered into
// 64-byte blocks (parts_gather.hpp) and compressed, its digest stored at out + 32 a.
// Shared by k_digest_parts (parts_kernels.hip: lanes in the caller's order) and
// k_digest_parts_planned (parts_plan.hip: lanes in the order planned on the GPU), which
// differ only in how a lane finds its action. Why the block under assembly lives in an
// LDS slot of the lane's own, 17 dwords from the next, is told in parts_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sha256_device.hpp"
#include "kernels.hpp"
#include "parts_gather.hpp"

namespace msha {

constexpr int kPartsSlotStride = 17;  // dwords, odd (parts_kernels.hip)

// slots: the workgroup's 256 x kPartsSlotStride dwords of LDS.
__device__ __forceinline__ void digest_parts_lane(const uint8_t* __restrict__ arena,
                                                  const uint64_t* __restrict__ part_off,
                                                  const uint64_t* __restrict__ part_len,
                                                  const uint64_t* __restrict__ begin, uint64_t a,
                                                  uint8_t* __restrict__ out, uint32_t* __restrict__ err,
                                                  uint32_t* slots) {
  const uint64_t j0 = begin[a], jend = begin[a + 1];
  // a decreasing part range (or one of 2^32 parts or more): flagged and zeroed, never a wrong digest
  if (jend < j0 || jend - j0 > 0xffffffffull) {
    uint8_t* o = out + 32 * a;
    atomicOr(err, kErrPartsBegin);
    reinterpret_cast<uint4*>(o)[0] = make_uint4(0, 0, 0, 0);
    reinterpret_cast<uint4*>(o)[1] = make_uint4(0, 0, 0, 0);
    return;
  }
  uint32_t* slot = slots + threadIdx.x * kPartsSlotStride;
  auto slot_write = [slot](uint32_t j, uint32_t v) { slot[j] = v; };
  auto load = [arena](uint64_t off) {
    uint4 v = *reinterpret_cast<const uint4*>(arena + off);
    // one 16-byte load: without this the compiler splits it by the dwords each byte
    // phase selects, into three overlapping 8-byte loads
    asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
    parts::Granule g;
    g.d[0] = v.x; g.d[1] = v.y; g.d[2] = v.z; g.d[3] = v.w;
    return g;
  };
  parts::Cursor c;
  parts::cursor_init(c, j0, (uint32_t)(jend - j0), part_off, part_len);

  State s;
  state_init(s);
  uint64_t total = 0;
  // 0: the stream's blocks, the padded tail included; 1: the length block after a
  // tail of 56 bytes or more; 2: done
  int phase = 0;
  while (phase != 2) {
    uint32_t w[16];
    if (phase == 0) {
      const uint32_t r = parts::fill_block(c, part_off, part_len, slot_write, load);
      total += r;
      uint32_t raw[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) raw[j] = slot[j];
      if (r == 64) {
        to_words(raw, w);
      } else {
        phase = build_tail(raw, r, total, w) ? 1 : 2;
      }
    } else {
      length_block(total, w);
      phase = 2;
    }
    compress(s, w);
  }
  store_digest(s, out + 32 * a);
}

}  // namespace msha
