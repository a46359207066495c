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

#include "kernels.hpp"
#include "parts_digest.hpp"

namespace msha {

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
  digest_parts_lane(arena, part_off, part_len, begin, a, out, err, slots);  // parts_digest.hpp
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
