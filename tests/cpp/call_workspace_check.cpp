// The workspace arithmetic of the device calls on the host, under AddressSanitizer +
// UBSan (tests/test_parts_route_cpu.py builds and runs this). Two parts:
//   layouts  parts_plan.hpp and parts_route.hpp Layout over every combination of n, m,
//            flat_bytes and with_list below, against the formulas written out here: every
//            offset and total, the arrays in order, disjoint and 64-byte aligned, the
//            buffer 256-byte aligned, the planned layout inside the routed one equal to
//            the stand-alone one shifted, and the order's offset independent of n;
//   growth   workspace_rule.hpp growth() for a need below, equal to and above the
//            capacity, on a capturing stream and off it.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../mirbft_amd/csrc/parts_route.hpp"

namespace pp = msha::parts_plan;
namespace pr = msha::parts_route;

namespace {

int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      ++failures;                        \
      std::printf("FAIL: " __VA_ARGS__); \
      std::printf("\n");                 \
    }                                    \
  } while (0)

uint64_t r64(uint64_t x) { return (x + 63) / 64 * 64; }
uint64_t r256(uint64_t x) { return (x + 255) / 256 * 256; }

// begin[i] .. begin[i] + size[i] in order, disjoint, 64-byte aligned, all inside `bytes`.
void check_arrays(const char* what, const uint64_t* begin, const uint64_t* size, int k, uint64_t bytes) {
  for (int i = 0; i < k; ++i) {
    CHECK(begin[i] % 64 == 0, "%s: array %d at %" PRIu64 " is not 64-byte aligned", what, i, begin[i]);
    CHECK(begin[i] + size[i] >= begin[i], "%s: array %d wraps", what, i);
    const uint64_t next = i + 1 < k ? begin[i + 1] : bytes;
    CHECK(begin[i] + size[i] <= next, "%s: array %d (%" PRIu64 " + %" PRIu64 ") runs past %" PRIu64, what, i, begin[i],
          size[i], next);
  }
}

}  // namespace

int main() {
  constexpr uint64_t kHead = 4 * (16 + 4148);  // info and the counters
  static_assert(pp::kKeys == 4148 && pr::kClaimWords == 8, "the formulas below are written for these");
  int n_layouts = 0;
  for (uint64_t n : {0ull, 1ull, 63ull, 64ull, 65ull, 4095ull, (1ull << 32) - 2}) {
    for (bool wl : {false, true}) {
      // the planned call's workspace
      const pp::Layout p(n, wl);
      const uint64_t order = r64(kHead), key16 = order + r64(4 * n), used = key16 + r64(2 * n),
                     table = used + (wl ? r64(n) : 0), bytes = table + (wl ? 32 * n : 0) + 64;
      CHECK(p.order == order && p.key16 == key16 && p.used == used && p.table == table && p.bytes == bytes,
            "planned n %" PRIu64 " list %d: %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64, n, (int)wl,
            p.order, p.key16, p.used, p.table, p.bytes);
      CHECK(p.order == pp::Layout(0, false).order && p.order == 16704, "the order's offset depends on n (%" PRIu64 ")", n);
      {
        const uint64_t begin[] = {0, p.order, p.key16, p.used, p.table};
        const uint64_t size[] = {kHead, 4 * n, 2 * n, wl ? n : 0, wl ? 32 * n : 0};
        check_arrays("planned", begin, size, 5, p.bytes);
      }
      ++n_layouts;
      for (uint64_t m : {1ull, 16ull, 4096ull}) {
        for (uint64_t fb : {16ull + 64, 4096ull, 1ull << 48}) {
          // the routed call's
          const pr::Layout l(n, m, fb, wl);
          const uint64_t claim = r64(kHead), msg_off = claim + r64(8 * 8), msg_len = msg_off + r64(8 * m),
                         sel = msg_len + r64(8 * m), chain = sel + r64(4 * m), out_idx = chain + r64(4 * m),
                         r_order = out_idx + r64(4 * m), r_key16 = r_order + r64(4 * n), r_used = r_key16 + r64(2 * n),
                         r_table = r_used + (wl ? r64(n) : 0), flat = r256(r_table + (wl ? 32 * n : 0) + 64),
                         r_bytes = flat + fb;
          CHECK(l.claim == claim && l.msg_off == msg_off && l.msg_len == msg_len && l.sel == sel && l.chain == chain &&
                    l.out_idx == out_idx && l.plan.order == r_order && l.plan.key16 == r_key16 &&
                    l.plan.used == r_used && l.plan.table == r_table && l.flat == flat && l.bytes == r_bytes,
                "routed n %" PRIu64 " m %" PRIu64 " flat %" PRIu64 " list %d", n, m, fb, (int)wl);
          const uint64_t shift = l.plan.order - p.order;
          CHECK(l.plan.key16 == p.key16 + shift && l.plan.used == p.used + shift && l.plan.table == p.table + shift &&
                    l.plan.bytes == p.bytes + shift,
                "routed n %" PRIu64 " m %" PRIu64 ": the planned layout inside is not the stand-alone one shifted", n, m);
          CHECK(l.flat % 256 == 0 && l.flat >= l.plan.bytes, "routed: flat at %" PRIu64, l.flat);
          const uint64_t begin[] = {0,         l.claim,      l.msg_off,    l.msg_len,   l.sel,        l.chain,
                                    l.out_idx, l.plan.order, l.plan.key16, l.plan.used, l.plan.table, l.flat};
          const uint64_t size[] = {kHead, 8 * 8, 8 * m, 8 * m, 4 * m, 4 * m, 4 * m, 4 * n, 2 * n, wl ? n : 0,
                                   wl ? 32 * n : 0, fb};
          check_arrays("routed", begin, size, 12, l.bytes);
          ++n_layouts;
        }
      }
    }
  }

  // growth: refuse exactly when capturing and need > capacity, grow exactly when not
  // capturing and need > capacity, to need + spare; otherwise nothing is allocated
  int n_growth = 0;
  for (uint64_t cap : {0ull, 1ull, 4096ull, 1ull << 40}) {
    for (uint64_t need : {cap ? cap - 1 : 0, cap, cap + 1, 2 * cap + 64}) {
      for (uint64_t spare : {uint64_t(0), need / 4, uint64_t(1) << 20}) {
        for (bool capturing : {false, true}) {
          const msha::Growth g = msha::growth(need, cap, spare, capturing);
          const bool more = need > cap;
          CHECK(g.refuse == (more && capturing) && g.grow == (more && !capturing),
                "need %" PRIu64 " cap %" PRIu64 " capturing %d: refuse %d grow %d", need, cap, (int)capturing,
                (int)g.refuse, (int)g.grow);
          CHECK(g.alloc == (g.grow ? need + spare : 0), "need %" PRIu64 " spare %" PRIu64 ": alloc %" PRIu64, need, spare,
                g.alloc);
          CHECK(!g.grow || g.alloc > cap, "need %" PRIu64 " cap %" PRIu64 ": the workspace shrinks to %" PRIu64, need,
                cap, g.alloc);
          ++n_growth;
        }
      }
    }
  }
  // a fresh workspace: any call refused under capture, grown otherwise
  CHECK(msha::growth(1, 0, 0, true).refuse && !msha::growth(1, 0, 0, true).grow, "fresh, capturing");
  CHECK(msha::growth(1, 0, 0, false).grow && !msha::growth(1, 0, 0, false).refuse && msha::growth(1, 0, 0, false).alloc == 1,
        "fresh, not capturing");
  if (failures) return 1;
  std::printf("call_workspace ok: %d layouts, %d growth decisions\n", n_layouts, n_growth);
  return 0;
}
