// The claim arithmetic of msha_hash_actions_device_routed (mirbft_amd/csrc/parts_route.hpp)
// on the host, under AddressSanitizer + UBSan (tests/test_parts_route_cpu.py builds and
// runs this). Two parts:
//   edges   is_long, slot_ok and room_ok at the values the caller gives on the command
//           line -- "given len long_bytes" triples -- printed for the test to compare
//           with its own restatement in Python integers (no 64-bit wrap there);
//   replay  k_route_measure's claim sequence, one list after the other, over equal and
//           mixed lengths under every cap: the counter is the exact sum of the rounded
//           lengths of what was routed and never passes long_bytes - slack, and for
//           equal lengths the count is min(n_long, max_long, floor(room / round16(L))).
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../mirbft_amd/csrc/parts_route.hpp"

namespace pr = msha::parts_route;
namespace pc = msha::parts_concat;

namespace {

constexpr uint64_t kSlack = 64;  // MSHA_DEVICE_ARENA_SLACK

int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      ++failures;                        \
      std::printf("FAIL: " __VA_ARGS__); \
      std::printf("\n");                 \
    }                                    \
  } while (0)

struct Routed {
  uint64_t count = 0, bytes = 0, tickets = 0;
};

// The kernel's sequence for one list after the other (the order the atomics settle).
Routed replay(const std::vector<uint64_t>& lens, uint32_t long_blocks, uint32_t max_long, uint64_t long_bytes) {
  Routed r;
  for (uint64_t len : lens) {
    const uint64_t blocks = (len >> 6) + ((len & 63) < 56 ? 1 : 2);
    uint64_t next = 0;
    if (!pr::is_long(blocks, long_blocks) || !pr::room_ok(0, len, long_bytes, kSlack, &next)) continue;
    const uint64_t ticket = r.tickets++;
    if (!pr::slot_ok(ticket, max_long)) continue;
    if (!pr::room_ok(r.bytes, len, long_bytes, kSlack, &next)) continue;
    CHECK(next == r.bytes + pc::round16(len) && next >= r.bytes, "next %" PRIu64 " after %" PRIu64, next, r.bytes);
    CHECK(next + kSlack <= long_bytes, "counter %" PRIu64 " + slack over long_bytes %" PRIu64, next, long_bytes);
    r.bytes = next;
    ++r.count;
  }
  return r;
}

}  // namespace

int main(int argc, char** argv) {
  static_assert(pr::kUnfilledLen == 0, "the copy skips a message of no bytes");
  static_assert(pr::kUnfilledOrder == 0xFFFFFFFFu, "the chain skips kNoLane");
  static_assert(pr::kClaimBytes < pr::kClaimWords && pr::kClaimSlots < pr::kClaimWords &&
                    pr::kClaimRouted < pr::kClaimWords,
                "the counters lie inside the claim words");
  // edges: given len long_bytes -> "E given len long_bytes ok next"
  int n_edges = 0;
  for (int i = 1; i + 2 < argc; i += 3) {
    const uint64_t given = std::strtoull(argv[i], nullptr, 10), len = std::strtoull(argv[i + 1], nullptr, 10),
                   bytes = std::strtoull(argv[i + 2], nullptr, 10);
    uint64_t next = 0;
    const bool ok = pr::room_ok(given, len, bytes, kSlack, &next);
    std::printf("E %" PRIu64 " %" PRIu64 " %" PRIu64 " %d %" PRIu64 "\n", given, len, bytes, ok ? 1 : 0,
                ok ? next : (uint64_t)0);
    ++n_edges;
  }
  // is_long and slot_ok at their edges
  for (uint32_t lb : {1u, 4u, 64u, 0xFFFFFFFFu}) {
    CHECK(pr::is_long(lb, lb) && pr::is_long((uint64_t)lb + 1, lb) && !pr::is_long((uint64_t)lb - 1, lb),
          "is_long at %u", lb);
    CHECK(pr::is_long(~0ull, lb), "is_long of 2^64 - 1 at %u", lb);
  }
  CHECK(!pr::slot_ok(0, 0) && pr::slot_ok(0, 1) && !pr::slot_ok(1, 1) && pr::slot_ok(4095, 4096) &&
            !pr::slot_ok(4096, 4096) && !pr::slot_ok(~0ull, 0xFFFFFFFFu),
        "slot_ok");

  // replay: equal lengths under every cap
  int n_replays = 0;
  for (uint64_t len : {1ull, 15ull, 16ull, 17ull, 1000ull, 1008ull, 91312ull}) {
    const uint64_t r16 = pc::round16(len);
    for (uint64_t n_long : {0ull, 1ull, 5ull, 70ull}) {
      for (uint32_t max_long : {1u, 2u, 5u, 4096u}) {
        for (uint64_t fit : {0ull, 1ull, 3ull, 5ull, 100ull}) {
          for (int64_t delta : {-1, 0, 1, 15}) {
            const uint64_t long_bytes = fit * r16 + kSlack + (uint64_t)delta;
            if ((int64_t)(fit * r16) + delta < 0) continue;
            const std::vector<uint64_t> lens(n_long, len);
            const Routed r = replay(lens, 1, max_long, long_bytes);
            uint64_t want = (long_bytes - kSlack) / r16;
            if (n_long < want) want = n_long;
            if (max_long < want) want = max_long;
            CHECK(r.count == want, "len %" PRIu64 " n %" PRIu64 " max %u bytes %" PRIu64 ": %" PRIu64 " routed, want %" PRIu64,
                  len, n_long, max_long, long_bytes, r.count, want);
            CHECK(r.bytes == r.count * r16, "bytes %" PRIu64 " for %" PRIu64 " lists of %" PRIu64, r.bytes, r.count, len);
            ++n_replays;
          }
        }
      }
    }
  }
  // mixed lengths: short ones never claim, long ones that fit both caps are all routed, and
  // a list larger than the whole buffer takes no slot from the others
  {
    const std::vector<uint64_t> lens = {10, 5000, 100, ~0ull, ~0ull - 14, 300, 1ull << 63, 7000, 183, 184};
    const Routed r = replay(lens, 4, 3, 5008 + 304 + 7008 + kSlack);
    CHECK(r.count == 3 && r.tickets == 4 && r.bytes == 5008 + 304 + 7008, "mixed: %" PRIu64 " routed, %" PRIu64 " tickets, %" PRIu64 " bytes",
          r.count, r.tickets, r.bytes);
    const Routed all = replay(lens, 4, 4, 5008 + 304 + 7008 + 192 + kSlack);
    CHECK(all.count == 4 && all.bytes == 5008 + 304 + 7008 + 192, "mixed, all fit: %" PRIu64 " routed", all.count);
    ++n_replays;
  }
  if (failures) return 1;
  std::printf("parts_route ok: %d edges, %d replays\n", n_edges, n_replays);
  return 0;
}
