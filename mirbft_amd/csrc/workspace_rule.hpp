// The arithmetic of a device call's workspace, without a HIP call: the rounding its
// layouts share (parts_plan.hpp, parts_route.hpp, stream_chain.hpp) and the decision of
// call_workspace.hpp CallWorkspace -- refuse, grow or keep -- as a pure function.
// Compiles for the host as well: tests/cpp/call_workspace_check.cpp runs it under
// AddressSanitizer + UBSan.
#pragma once
#include <stdint.h>

#include "parts_gather.hpp"

namespace msha {

MSHA_HD uint64_t round64(uint64_t x) { return (x + 63) & ~uint64_t(63); }
MSHA_HD uint64_t round256(uint64_t x) { return (x + 255) & ~uint64_t(255); }

// A call needs `need` bytes of a workspace that holds `capacity`. A capturing stream
// allows no allocation, so there a larger need is refused; elsewhere the workspace grows
// to need + spare. It never shrinks. alloc: the bytes to allocate when grow, else 0.
struct Growth {
  bool refuse, grow;
  uint64_t alloc;
};
MSHA_HD Growth growth(uint64_t need, uint64_t capacity, uint64_t spare, bool capturing) {
  const bool more = need > capacity;
  return Growth{more && capturing, more && !capturing, more && !capturing ? need + spare : 0};
}

}  // namespace msha
