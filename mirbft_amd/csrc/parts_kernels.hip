// Multi-part actions hashed from HBM (gfx950 only): msha_hash_actions_device.
//
// ProcessHashActions (pkg/processor/serial.go:180-198) hashes an action's Data as a
// list of byte slices written back to back; an EpochChange's Data interleaves 8-byte
// big-endian fields with 32-byte digests (pkg/statemachine/stateless.go:323-352). The
// other device entries want each message contiguous and 16-byte aligned
// (k_digest_batch) or made of 32-byte rows of one table (k_digest_of_digests). Here
// one lane assembles its action's 64-byte blocks from byte-granular, arbitrarily
// aligned parts (parts_gather.hpp) and compresses them.
//
// A lane stages the block it is assembling in an LDS slot of its own: its fill
// position differs from lane to lane, and a register array indexed by it would go to
// scratch. Slots are 17 dwords apart: ds_read_b32 and ds_write_b32 bank by dword
// address mod 32 within each 32-lane half of the wave, and 17 is odd, so the read-back
// of dword j at a static index touches 32 different banks per half (a stride of 16 or
// 32 would put every lane on one or two banks). The gather's writes go to lane-dependent
// indices and conflict as the data has it. 256 lanes x 68 B = 17 KB a workgroup, 8
// workgroups a CU within the 160 KB. No lane reads another's slot: there is no
// barrier and no wave waits on another.
//
// The gather loop is divergent (lanes take different numbers of steps); the
// compression is not: the block loop has one compress() call site, and the lanes
// that still have a block reach it together.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sha256_device.hpp"
#include "kernels.hpp"
#include "parts_gather.hpp"

namespace msha {

constexpr int kPartsSlotStride = 17;  // dwords, odd (see above)

__global__ __launch_bounds__(256, 8) void k_digest_parts(const uint8_t* __restrict__ arena,
                                                        const uint64_t* __restrict__ part_off,
                                                        const uint64_t* __restrict__ part_len,
                                                        const uint64_t* __restrict__ begin,
                                                        const uint32_t* __restrict__ order, uint64_t n,
                                                        uint8_t* __restrict__ out, uint32_t* __restrict__ err) {
  __shared__ uint32_t slots[256 * kPartsSlotStride];
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t a = order ? (uint64_t)order[i] : i;
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

hipError_t launch_digest_parts(const uint8_t* arena, const uint64_t* part_off, const uint64_t* part_len,
                               const uint64_t* begin, const uint32_t* order, uint64_t n, uint8_t* out,
                               uint32_t* err, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_digest_parts, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, arena, part_off,
                     part_len, begin, order, n, out, err);
  return hipGetLastError();
}

}  // namespace msha
