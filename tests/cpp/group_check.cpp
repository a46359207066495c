// Stand-alone check of mirbft_amd/csrc/group.hpp (tests/test_group_cpu.py builds it with
// -fsanitize=address,undefined and runs it). The header is what the six kernels of
// msha_group_digests_device run; here the lanes run one after the other, plain loads and
// stores stand in for the three atomic operations, and callbacks for the tile table and
// the workgroup prefix.
//
// Every array is a heap block of exactly its contract size: 32 n bytes of digests, 4 n of
// scopes, n entries each of first, group and members, group_cap entries of the two group
// arrays, and of the workspace capacity(n) table entries, n positions, counts and ids and
// tiles(n) totals. So a row read past n, a table position past the capacity or a group
// entry at or past group_cap is an AddressSanitizer report.
//
// The insert runs in three slot orders -- ascending, descending and a fixed shuffle --
// and every output must be the same in all three: the answer does not depend on the order
// the lanes ran in. The first order's outputs go to the result file, which the pytest
// file compares with its numpy oracle.
//
// argv[1]: the cases tests/group_matrix.py wrote (write_cases); argv[2]: where the
// results go (per case the five result words, first, group, members, group_first,
// group_count). A line a case is printed as well, and before the cases the workspace
// layout is checked over a range of sizes.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mirbft_amd/csrc/group.hpp"

namespace gp = msha::group;

typedef unsigned long long ull;

static int g_failed = 0;
static uint64_t g_case = 0;
#define CHECK(cond, ...)                                                     \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("FAIL case %llu:%d: %s: ", (ull)g_case, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                              \
      std::printf("\n");                                                     \
      ++g_failed;                                                            \
    }                                                                        \
  } while (0)

static const uint32_t kSentinel = 0xA5A5A5A5u;
static const uint32_t kFlip = 0x5A;
static const uint64_t kSeed = 0x0123456789ABCDEFull;

// tests/group_matrix.py base_rows
static void base_row(uint64_t r, uint8_t* row) {
  for (uint32_t j = 0; j < 8; ++j) {
    const uint32_t w = (uint32_t)(r * 0x9E3779B1ull + j * 0x85EBCA6Bull);
    std::memcpy(row + 4 * j, &w, 4);
  }
}

template <class T>
static T* exact(uint64_t count) {
  return static_cast<T*>(std::malloc(count * sizeof(T)));  // count 0: a block of no bytes
}

static bool read_words(std::FILE* f, void* dst, uint64_t bytes) {
  const uint64_t padded = (bytes + 7u) & ~uint64_t(7);
  std::vector<uint8_t> buf(padded);
  if (padded && std::fread(buf.data(), 1, padded, f) != padded) return false;
  if (bytes) std::memcpy(dst, buf.data(), bytes);
  return true;
}

struct Inputs {
  uint64_t n = 0, group_cap = 0;
  const uint8_t* digests = nullptr;
  const uint32_t* scope = nullptr;
  bool force_home = false;
  uint64_t force_at = 0;
};

struct Outputs {
  uint32_t *first, *group, *members, *group_first, *group_count;
  uint64_t r[5];
  Outputs(uint64_t n, uint64_t cap)
      : first(exact<uint32_t>(n)), group(exact<uint32_t>(n)), members(exact<uint32_t>(n)),
        group_first(exact<uint32_t>(cap)), group_count(exact<uint32_t>(cap)) {
    for (uint64_t i = 0; i < n; ++i) first[i] = group[i] = members[i] = kSentinel;
    for (uint64_t g = 0; g < cap; ++g) group_first[g] = group_count[g] = kSentinel;
    std::memset(r, 0xFF, sizeof r);
  }
  ~Outputs() {
    std::free(first);
    std::free(group);
    std::free(members);
    std::free(group_first);
    std::free(group_count);
  }
  Outputs(const Outputs&) = delete;
  Outputs& operator=(const Outputs&) = delete;
};

static gp::Key key_of(const Inputs& in, uint64_t s) {
  gp::Key k;
  k.scope = in.scope ? in.scope[s] : 0u;
  std::memcpy(k.lo.d, in.digests + 32 * s, 16);
  std::memcpy(k.hi.d, in.digests + 32 * s + 16, 16);
  return k;
}

// The six kernels over one case, the insert's lanes in `order`. Returns the longest probe.
static uint64_t run(const Inputs& in, const std::vector<uint32_t>& order, Outputs* out) {
  const uint64_t n = in.n;
  const gp::Layout lay(n);
  const uint64_t tiles = gp::tiles(n);
  uint32_t* const table = exact<uint32_t>(lay.cap);
  uint32_t* const pos = exact<uint32_t>(n);
  uint32_t* const count = exact<uint32_t>(n);
  uint32_t* const id = exact<uint32_t>(n);
  uint32_t* const totals = exact<uint32_t>(tiles);

  // k_group_init
  for (uint64_t p = 0; p < lay.cap; ++p) table[p] = gp::kEmpty;
  for (uint64_t i = 0; i < n; ++i) count[i] = 0;
  uint64_t best = 0;
  for (uint64_t i = 0; i < n; ++i) pos[i] = id[i] = kSentinel;

  // k_group_insert
  gp::Placement pl;
  pl.seed = kSeed;
  pl.mask = (uint32_t)(lay.cap - 1);
  pl.force_home = in.force_home ? 1u : 0u;
  pl.force_at = (uint32_t)(in.force_at % lay.cap);
  uint64_t longest = 0;
  for (uint32_t i : order) {
    const gp::Key k = key_of(in, i);
    uint64_t steps = 0;
    pos[i] = gp::probe(
        i, gp::home(pl, k), pl.mask,
        [&](uint32_t p) {
          ++steps;
          return table[p];
        },
        [&](uint32_t p, uint32_t me) {
          const uint32_t old = table[p];
          if (old == gp::kEmpty) table[p] = me;
          return old;
        },
        [&](uint32_t p, uint32_t me) {
          if (me < table[p]) table[p] = me;
        },
        [&](uint32_t j) {
          CHECK(j < n, "slot %u compares with owner %u", i, j);
          return j < n && gp::same(k, key_of(in, j));
        });
    CHECK(steps <= lay.cap, "slot %u took %llu steps", i, (ull)steps);
    longest = steps > longest ? steps : longest;
  }

  // k_group_resolve, a tile a workgroup
  for (uint64_t tile = 0; tile < tiles; ++tile) {
    uint32_t t_key[gp::kTileSlots], t_cnt[gp::kTileSlots];
    for (uint32_t j = 0; j < gp::kTileSlots; ++j) {
      t_key[j] = gp::kEmpty;
      t_cnt[j] = 0;
    }
    uint32_t leaders = 0;
    for (uint64_t i = tile * gp::kTile; i < n && i < (tile + 1) * gp::kTile; ++i) {
      const uint32_t first = table[pos[i]];
      CHECK(first <= i, "slot %llu follows %u", (ull)i, first);
      out->first[i] = first;
      if (first == i) ++leaders;
      const uint32_t h = gp::tile_slot(
          first, [&](uint32_t s) { return t_key[s]; },
          [&](uint32_t s, uint32_t me) {
            const uint32_t old = t_key[s];
            if (old == gp::kEmpty) t_key[s] = me;
            return old;
          });
      t_cnt[h]++;
    }
    // one add a leader and tile: no leader owns two entries of the tile table
    std::vector<uint32_t> owners;
    for (uint32_t j = 0; j < gp::kTileSlots; ++j) {
      if (t_key[j] == gp::kEmpty) continue;
      owners.push_back(t_key[j]);
      count[t_key[j]] += t_cnt[j];
    }
    std::sort(owners.begin(), owners.end());
    for (size_t j = 1; j < owners.size(); ++j) CHECK(owners[j - 1] != owners[j], "leader %u in two tile entries", owners[j]);
    totals[tile] = leaders;
  }

  // k_group_scan: the workgroup prefix of each chunk, then every thread's walk
  const uint64_t chunks = (tiles + gp::kScanTiles - 1) / gp::kScanTiles;
  std::vector<uint32_t> before(chunks * gp::kScanThreads), all(chunks);
  for (uint64_t c = 0; c < chunks; ++c) {
    uint32_t sum = 0;
    for (uint32_t t = 0; t < gp::kScanThreads; ++t) {
      before[c * gp::kScanThreads + t] = sum;
      const uint64_t k = c * gp::kScanTiles + t;
      if (k < tiles) sum += totals[k];
    }
    all[c] = sum;
  }
  std::vector<uint8_t> stored(tiles, 0);
  uint64_t groups = 0;
  for (uint32_t t = 0; t < gp::kScanThreads; ++t) {
    uint64_t chunk = 0;
    const uint64_t g = gp::scan_walk(
        tiles, t, [&](uint64_t k) { return totals[k]; },
        [&](uint32_t c, uint32_t* bf, uint32_t* al) {
          (void)c;
          *bf = before[chunk * gp::kScanThreads + t];
          *al = all[chunk];
          ++chunk;
        },
        [&](uint64_t k, uint32_t b) {
          totals[k] = b;
          stored[k]++;
        });
    CHECK(chunk == chunks, "thread %u asked for %llu prefixes of %llu", t, (ull)chunk, (ull)chunks);
    if (t == 0) groups = g;
    CHECK(g == groups, "thread %u counts %llu groups, thread 0 %llu", t, (ull)g, (ull)groups);
  }
  for (uint64_t k = 0; k < tiles; ++k) CHECK(stored[k] == 1, "tile base %llu stored %d times", (ull)k, stored[k]);

  // k_group_rank
  std::vector<uint8_t> listed(in.group_cap, 0);
  const uint64_t limit = groups < in.group_cap ? groups : in.group_cap;
  for (uint64_t tile = 0; tile < tiles; ++tile) {
    uint64_t ballots[gp::kTileWaves] = {};
    for (uint32_t t = 0; t < gp::kTile; ++t) {
      const uint64_t i = tile * gp::kTile + t;
      if (i < n && out->first[i] == i) ballots[t >> 6] |= uint64_t(1) << (t & 63u);
    }
    for (uint32_t t = 0; t < gp::kTile; ++t) {
      const uint64_t i = tile * gp::kTile + t;
      if (!(i < n && out->first[i] == i)) continue;
      const uint32_t g = totals[tile] + gp::rank_in_tile(ballots, t >> 6, t & 63u);
      id[i] = g;
      if (g < in.group_cap) {
        if (g >= limit) {  // not performed: the contract is already broken
          CHECK(g < limit, "group %u listed, min(groups, group_cap) is %llu", g, (ull)limit);
          continue;
        }
        CHECK(listed[g] == 0, "group %u listed twice", g);
        listed[g] = 1;
        out->group_first[g] = (uint32_t)i;
        out->group_count[g] = count[i];
      }
      const uint64_t key = gp::best_key(count[i], g);
      CHECK(key != 0, "a group's key is 0");
      best = key > best ? key : best;
    }
  }

  // k_group_fill
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t f = out->first[i];
    out->group[i] = id[f];
    out->members[i] = count[f];
  }
  gp::result_words(n, groups, in.group_cap, best, out->r);

  std::free(table);
  std::free(pos);
  std::free(count);
  std::free(id);
  std::free(totals);
  return longest;
}

static bool same_outputs(const Outputs& a, const Outputs& b, uint64_t n, uint64_t cap) {
  return std::memcmp(a.r, b.r, sizeof a.r) == 0 && (n == 0 || (std::memcmp(a.first, b.first, 4 * n) == 0 &&
                                                               std::memcmp(a.group, b.group, 4 * n) == 0 &&
                                                               std::memcmp(a.members, b.members, 4 * n) == 0)) &&
         (cap == 0 || (std::memcmp(a.group_first, b.group_first, 4 * cap) == 0 &&
                       std::memcmp(a.group_count, b.group_count, 4 * cap) == 0));
}

static void write_u32(std::FILE* f, const uint32_t* a, uint64_t count) {
  std::fwrite(a, 4, count, f);
  if (count & 1u) {
    const uint32_t pad = 0;
    std::fwrite(&pad, 4, 1, f);
  }
}

// capacity a power of two, at least 2 n and one wave's worth; the arrays in order, each
// 256-aligned and large enough, none overlapping the next.
static void check_layout() {
  std::vector<uint64_t> ns = {1, 2, 3, 31, 32, 33, 63, 64, 65, 300, 4097};
  for (uint32_t b = 7; b <= 30; ++b) {
    ns.push_back((uint64_t(1) << b) - 1);
    ns.push_back(uint64_t(1) << b);
    if (b < 30) ns.push_back((uint64_t(1) << b) + 1);
  }
  for (uint64_t n : ns) {
    const gp::Layout lay(n);
    CHECK(lay.cap == gp::capacity(n) && (lay.cap & (lay.cap - 1)) == 0, "n %llu: capacity %llu", (ull)n, (ull)lay.cap);
    CHECK(lay.cap >= 2 * n && lay.cap >= gp::kMinCapacity && lay.cap <= (uint64_t(1) << 31), "n %llu: capacity %llu",
          (ull)n, (ull)lay.cap);
    CHECK(lay.cap == gp::kMinCapacity || lay.cap < 4 * n, "n %llu: capacity %llu is more than bit_ceil(2 n)", (ull)n,
          (ull)lay.cap);
    const uint64_t at[7] = {lay.head, lay.table, lay.pos, lay.count, lay.id, lay.totals, lay.bytes};
    const uint64_t need[6] = {16, 4 * lay.cap, 4 * n, 4 * n, 4 * n, 4 * gp::tiles(n)};
    for (uint32_t k = 0; k < 6; ++k) {
      CHECK(at[k] % 256 == 0, "n %llu: array %u at %llu", (ull)n, k, (ull)at[k]);
      CHECK(at[k] + need[k] <= at[k + 1], "n %llu: array %u overlaps the next", (ull)n, k);
    }
    // k_group_init clears the counters four at a time
    CHECK(lay.count + 16 * ((n + 3) / 4) <= lay.id && (n + 3) / 4 <= lay.cap / 4, "n %llu: the counters' quarter", (ull)n);
  }
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::printf("usage: group_check CASES RESULTS\n");
    return 2;
  }
  std::FILE* in_f = std::fopen(argv[1], "rb");
  std::FILE* out_f = std::fopen(argv[2], "wb");
  uint64_t count = 0;
  if (!in_f || !out_f || std::fread(&count, 8, 1, in_f) != 1) {
    std::printf("cannot open the case or the result file\n");
    return 2;
  }
  g_case = ~uint64_t(0);
  check_layout();
  std::printf("layout checked\n");

  for (uint64_t k = 0; k < count; ++k) {
    g_case = k;
    int64_t h[6];
    if (std::fread(h, 8, 6, in_f) != 6) return 2;
    const uint64_t n = (uint64_t)h[0], cap = (uint64_t)h[2], n_flips = (uint64_t)h[3];
    const bool has_scope = h[1] != 0;

    std::vector<uint32_t> val(n), flips(2 * n_flips);
    if (!read_words(in_f, val.data(), 4 * n)) return 2;
    uint32_t* const scope = has_scope ? exact<uint32_t>(n) : nullptr;
    if (has_scope && !read_words(in_f, scope, 4 * n)) return 2;
    if (!read_words(in_f, flips.data(), 8 * n_flips)) return 2;

    uint8_t* const digests = exact<uint8_t>(32 * n);
    for (uint64_t i = 0; i < n; ++i) base_row(val[i], digests + 32 * i);
    for (uint64_t j = 0; j < n_flips; ++j) digests[32ull * flips[2 * j] + flips[2 * j + 1]] ^= kFlip;

    Inputs in;
    in.n = n;
    in.group_cap = cap;
    in.digests = digests;
    in.scope = scope;
    in.force_home = h[4] >= 0;
    in.force_at = h[4] >= 0 ? (uint64_t)h[4] : 0;

    // ascending, descending, and a Fisher-Yates shuffle driven by a fixed LCG
    std::vector<uint32_t> up(n), down(n), mixed(n);
    for (uint64_t i = 0; i < n; ++i) {
      up[i] = mixed[i] = (uint32_t)i;
      down[i] = (uint32_t)(n - 1 - i);
    }
    uint64_t lcg = 0x2545F4914F6CDD1Dull + k;
    for (uint64_t i = n; i > 1; --i) {
      lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
      const uint64_t j = (lcg >> 33) % i;
      const uint32_t tmp = mixed[i - 1];
      mixed[i - 1] = mixed[j];
      mixed[j] = tmp;
    }

    Outputs a(n, cap), b(n, cap), c(n, cap);
    const uint64_t longest = run(in, up, &a);
    run(in, down, &b);
    run(in, mixed, &c);
    CHECK(same_outputs(a, b, n, cap), "the descending insert gives another answer");
    CHECK(same_outputs(a, c, n, cap), "the shuffled insert gives another answer");
    // a forced home makes one chain of all the keys: the last distinct key walks past the others
    if (in.force_home) CHECK(longest >= a.r[1], "forced home: longest probe %llu, %llu groups", (ull)longest, (ull)a.r[1]);

    std::printf("case %llu: n %llu groups %llu listed %llu max_count %llu max_group %llu\n", (ull)k, (ull)a.r[0],
                (ull)a.r[1], (ull)a.r[2], (ull)a.r[3], (ull)a.r[4]);
    std::fwrite(a.r, 8, 5, out_f);
    write_u32(out_f, a.first, n);
    write_u32(out_f, a.group, n);
    write_u32(out_f, a.members, n);
    write_u32(out_f, a.group_first, cap);
    write_u32(out_f, a.group_count, cap);
    std::free(scope);
    std::free(digests);
  }
  std::fclose(in_f);
  std::fclose(out_f);
  if (g_failed) {
    std::printf("group FAILED: %d checks\n", g_failed);
    return 1;
  }
  std::printf("group ok: %llu cases\n", (ull)count);
  return 0;
}
