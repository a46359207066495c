// The workspace layout of msha_dstreams_write_jobs_routed_device on the host, under
// AddressSanitizer + UBSan (tests/test_dstream_jobs_route_cpu.py builds and runs this):
// mirbft_amd/csrc/stream_jobs_route.hpp Layout over every combination of k jobs, n
// streams, m slots and flat_bytes below --
//   the jobs call's layout first and unchanged, the routed write's behind it at a
//   256-byte boundary and unchanged but for the shift; every array of either in order,
//   disjoint, 64-byte aligned, inside its own half; the flatten buffer last and 256-byte
//   (so 16-byte) aligned; bytes and arrays as documented;
//   ok at the largest arguments the entry admits, not ok where a size cannot fit or a
//   sub-layout refuses;
//   workspace_rule.hpp growth() on these sizes: a quarter of the arrays to spare, nothing
//   for the buffer, refused under capture exactly when the call needs more.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../mirbft_amd/csrc/stream_jobs_route.hpp"

namespace sj = msha::sjobs;
namespace sc = msha::schain;
namespace jr = msha::sjroute;

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

// begin[i] .. begin[i] + size[i] in order, disjoint, 64-byte aligned, all inside [lo, hi).
void check_arrays(const char* what, const uint64_t* begin, const uint64_t* size, int k, uint64_t lo, uint64_t hi) {
  CHECK(begin[0] >= lo, "%s: array 0 at %" PRIu64 " starts before %" PRIu64, what, begin[0], lo);
  for (int i = 0; i < k; ++i) {
    CHECK(begin[i] % 64 == 0, "%s: array %d at %" PRIu64 " is not 64-byte aligned", what, i, begin[i]);
    CHECK(begin[i] + size[i] >= begin[i], "%s: array %d wraps", what, i);
    const uint64_t next = i + 1 < k ? begin[i + 1] : hi;
    CHECK(begin[i] + size[i] <= next, "%s: array %d (%" PRIu64 " + %" PRIu64 ") runs past %" PRIu64, what, i, begin[i],
          size[i], next);
  }
}

}  // namespace

int main() {
  constexpr unsigned long long kMost = (1ull << 32) - 2;  // jobs a call, streams a set
  int n_layouts = 0;
  for (uint64_t k : {1ull, 2047ull, 2048ull, 2049ull, 100000ull, kMost}) {
    for (uint64_t n : {1ull, 4ull, 255ull, 256ull, 65536ull, kMost}) {
      for (uint64_t m : {1ull, 64ull, 4096ull}) {
        for (uint64_t fb : {16ull + 64, 4096ull, 32ull << 20, 1ull << 48}) {
          const jr::Layout l(k, n, m, fb);
          const sj::Layout j(k, n);
          const sc::Layout r(n, m, fb);
          CHECK(l.ok && j.ok && r.ok, "k %" PRIu64 " n %" PRIu64 " m %" PRIu64 " flat %" PRIu64 ": not ok", k, n, m, fb);
          if (!l.ok) continue;
          // the jobs call's layout, as it stands alone
          CHECK(l.jobs.pairs[0] == j.pairs[0] && l.jobs.pairs[1] == j.pairs[1] && l.jobs.off == j.off &&
                    l.jobs.len == j.len && l.jobs.counts == j.counts && l.jobs.begin == j.begin &&
                    l.jobs.bytes == j.bytes && l.jobs.n_tiles == j.n_tiles && l.jobs.n_counts == j.n_counts,
                "k %" PRIu64 " n %" PRIu64 ": the jobs layout inside is not the stand-alone one", k, n);
          {
            const uint64_t begin[] = {j.pairs[0], j.pairs[1], j.off, j.len, j.counts, j.begin};
            const uint64_t size[] = {8 * k, 8 * k, 8 * k, 8 * k, 4 * j.n_counts, 8 * (n + 1)};
            check_arrays("jobs", begin, size, 6, 0, l.route_at);
          }
          // the routed write's, shifted
          CHECK(l.route_at % 256 == 0 && l.route_at >= j.bytes && l.route_at < j.bytes + 256, "route_at %" PRIu64,
                l.route_at);
          CHECK(l.claim == l.route_at + r.claim && l.taken == l.route_at + r.taken &&
                    l.slot_row == l.route_at + r.slot_row && l.slot_stream == l.route_at + r.slot_stream &&
                    l.slot_t == l.route_at + r.slot_t && l.msg_off == l.route_at + r.msg_off &&
                    l.msg_len == l.route_at + r.msg_len && l.blocks == l.route_at + r.blocks &&
                    l.flat == l.route_at + r.flat && l.bytes == l.route_at + r.bytes,
                "k %" PRIu64 " n %" PRIu64 " m %" PRIu64 ": the route layout inside is not the stand-alone one shifted",
                k, n, m);
          CHECK(l.route.flat == r.flat && l.route.bytes == r.bytes && l.route.claim == r.claim, "route sub-layout");
          {
            const uint64_t begin[] = {l.claim,   l.taken,   l.slot_row, l.slot_stream, l.slot_t,
                                      l.msg_off, l.msg_len, l.blocks,   l.flat};
            const uint64_t size[] = {8 * msha::parts_route::kClaimWords, (n + 3) / 4 * 4, 4 * m, 4 * m, 4 * m, 8 * m,
                                     8 * m, 8 * m, fb};
            check_arrays("route", begin, size, 9, l.route_at, l.bytes);
          }
          CHECK(l.flat % 256 == 0 && l.flat % 16 == 0, "the flatten buffer at %" PRIu64 " is not aligned", l.flat);
          CHECK(l.bytes == l.flat + fb && l.arrays == l.bytes - fb && l.arrays == l.flat, "bytes %" PRIu64 " arrays %" PRIu64,
                l.bytes, l.arrays);
          ++n_layouts;

          // growth on these sizes
          const uint64_t spare = l.arrays / 4;
          const msha::Growth fresh = msha::growth(l.bytes, 0, spare, false);
          CHECK(fresh.grow && !fresh.refuse && fresh.alloc == l.bytes + spare, "fresh: alloc %" PRIu64, fresh.alloc);
          CHECK(fresh.alloc - l.bytes == l.flat / 4, "the spare counts the flatten buffer");
          CHECK(msha::growth(l.bytes, 0, spare, true).refuse, "fresh and capturing: not refused");
          const msha::Growth same = msha::growth(l.bytes, fresh.alloc, spare, true);
          CHECK(!same.refuse && !same.grow && same.alloc == 0, "the same call again, capturing");
          // one job more on a workspace of exactly this call's size: refused only where it needs more
          const jr::Layout more(k + 1, n, m, fb);
          if (more.ok) {
            const msha::Growth g = msha::growth(more.bytes, l.bytes, more.arrays / 4, true);
            CHECK(g.refuse == (more.bytes > l.bytes), "a larger call on a capturing stream");
          }
          const jr::Layout wider(k, n, m, fb + 16);
          if (wider.ok) {
            CHECK(msha::growth(wider.bytes, l.bytes, wider.arrays / 4, true).refuse, "a larger buffer, capturing");
            CHECK(msha::growth(wider.bytes, l.bytes, wider.arrays / 4, false).alloc == wider.bytes + wider.arrays / 4,
                  "a larger buffer");
          }
        }
      }
    }
  }

  // the largest call the entry admits
  {
    const jr::Layout l(kMost, kMost, 16 * 4096, 1ull << 48);
    CHECK(l.ok && l.bytes > (1ull << 48) && l.bytes < (1ull << 50), "the largest call: ok %d bytes %" PRIu64, (int)l.ok,
          l.bytes);
  }
  // sizes that cannot fit, and arguments a sub-layout refuses
  int n_refused = 0;
  for (uint64_t k : std::initializer_list<uint64_t>{1ull << 61, UINT64_MAX / 8 + 1, UINT64_MAX - 1, UINT64_MAX}) {
    CHECK(!jr::Layout(k, 4, 64, 4096).ok, "k %" PRIu64 " is not refused", k);
    ++n_refused;
  }
  for (uint64_t n : std::initializer_list<uint64_t>{1ull << 32, 1ull << 61, UINT64_MAX}) {
    CHECK(!jr::Layout(100, n, 64, 4096).ok, "n %" PRIu64 " is not refused", n);
    ++n_refused;
  }
  CHECK(!jr::Layout(100, 4, 1ull << 32, 4096).ok, "m 2^32 is not refused");
  CHECK(!jr::Layout(100, 4, 64, (1ull << 48) + 1).ok, "flat_bytes above 2^48 is not refused");
  CHECK(!jr::Layout(100, 4, 64, UINT64_MAX).ok, "flat_bytes 2^64 - 1 is not refused");
  n_refused += 3;
  {
    const jr::Layout bad(UINT64_MAX, 4, 64, 4096);
    CHECK(bad.bytes == 0 && bad.flat == 0 && bad.route_at == 0, "a refused layout leaves offsets");
  }
  if (failures) return 1;
  std::printf("stream_jobs_route ok: %d layouts, %d refused\n", n_layouts, n_refused);
  return 0;
}
