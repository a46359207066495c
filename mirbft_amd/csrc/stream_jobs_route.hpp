// The workspace of msha_dstreams_write_jobs_routed_device (stream_device.cpp): the jobs
// call's arrays (stream_jobs.hpp Layout) first, and behind them, at a 256-byte boundary,
// the routed write's (stream_chain.hpp Layout) over the set's n streams -- the grouped
// CSR names every stream, so the routed write runs with n_rows == n. Neither sub-layout
// changes: each is the stand-alone one, the second shifted by route_at. The flatten
// buffer is the last array, 256-byte aligned from the workspace's base (16 is what the
// copy and the chain need).
//
// This header compiles for the host as well: tests/cpp/stream_jobs_route_check.cpp runs
// it under AddressSanitizer + UBSan.
#pragma once
#include <stdint.h>

#include "stream_chain.hpp"
#include "stream_jobs.hpp"
#include "workspace_rule.hpp"

namespace msha {
namespace sjroute {

// Byte offsets from the workspace's base for a call of k jobs on a set of n streams with
// m slots and a flatten buffer of flat_bytes. jobs: offsets from the base. route: offsets
// from route_at; claim .. flat are the same from the base. arrays: everything but the
// flatten buffer, what the workspace grows a quarter of to spare. ok is false where a
// size does not fit 64 bits or a sub-layout refuses its arguments.
struct Layout {
  sjobs::Layout jobs;
  schain::Layout route;
  uint64_t route_at = 0;
  uint64_t claim = 0, taken = 0, slot_row = 0, slot_stream = 0, slot_t = 0, msg_off = 0, msg_len = 0, blocks = 0,
           flat = 0;
  uint64_t arrays = 0, bytes = 0;
  bool ok = false;

  Layout(uint64_t k, uint64_t n, uint64_t m, uint64_t flat_bytes) : jobs(k, n), route(n, m, flat_bytes) {
    if (!jobs.ok || !route.ok) return;
    if (jobs.bytes > UINT64_MAX - 255) return;
    route_at = round256(jobs.bytes);
    if (route.bytes > UINT64_MAX - route_at) return;
    claim = route_at + route.claim;
    taken = route_at + route.taken;
    slot_row = route_at + route.slot_row;
    slot_stream = route_at + route.slot_stream;
    slot_t = route_at + route.slot_t;
    msg_off = route_at + route.msg_off;
    msg_len = route_at + route.msg_len;
    blocks = route_at + route.blocks;
    flat = route_at + route.flat;
    bytes = route_at + route.bytes;
    arrays = bytes - flat_bytes;
    ok = true;
  }
};

}  // namespace sjroute
}  // namespace msha
