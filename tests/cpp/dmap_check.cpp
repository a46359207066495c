// Stand-alone check of mirbft_amd/csrc/dmap.hpp (tests/test_dmap_cpu.py builds it with
// -fsanitize=address,undefined and runs it). The header is what the kernels of a device
// digest map run; here the lanes run one after the other, and plain loads and stores stand
// in for the atomic load and the compare-and-swap.
//
// Every array is a heap block of exactly its contract size: of the caller's, 32 n bytes of
// digests, 4 n of scopes, n entries each of id, before and after, crossed_cap entries of
// the crossed list; of the map, capacity(max_keys) table entries, max_keys scopes, 32
// max_keys digest bytes and max_keys counts; of the call's workspace, n entries each of
// first, members, and the leaders' id, position and before, and tiles(n) totals twice. So
// a stored key read past max_keys, a table position past the capacity or a crossed entry
// at or past crossed_cap is an AddressSanitizer report.
//
// Each sequence runs on three maps: the lanes of the call's insert and of the commit go in
// ascending, descending and a fixed shuffled order. After every step every output and
// everything msha_dmap_read would return must be the same on all three (where an id lies
// in the table may differ, and does). A refused add must leave every byte of the map as it
// was. The first map's outputs go to the result file, which the pytest file compares with
// its dict oracle.
//
// argv[1]: the sequences tests/dmap_matrix.py wrote (write_sequences); argv[2]: where the
// results go (read_results).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mirbft_amd/csrc/dmap.hpp"

namespace gp = msha::group;
namespace dm = msha::dmap;

typedef unsigned long long ull;

static int g_failed = 0;
static uint64_t g_seq = 0, g_step = 0;
#define CHECK(cond, ...)                                                                        \
  do {                                                                                          \
    if (!(cond)) {                                                                              \
      std::printf("FAIL sequence %llu step %llu:%d: %s: ", (ull)g_seq, (ull)g_step, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                                                 \
      std::printf("\n");                                                                        \
      ++g_failed;                                                                               \
    }                                                                                           \
  } while (0)

static const uint32_t kSentinel = 0xA5A5A5A5u;
static const uint32_t kFlip = 0x5A;
static const uint64_t kCallSeed = 0x0123456789ABCDEFull;
enum { kAdd = 0, kFind = 1, kClear = 2 };

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
template <class T>
static T* exact_filled(uint64_t count, T v) {
  T* p = exact<T>(count);
  for (uint64_t i = 0; i < count; ++i) p[i] = v;
  return p;
}

static bool read_words(std::FILE* f, void* dst, uint64_t bytes) {
  const uint64_t padded = (bytes + 7u) & ~uint64_t(7);
  std::vector<uint8_t> buf(padded);
  if (padded && std::fread(buf.data(), 1, padded, f) != padded) return false;
  if (bytes) std::memcpy(dst, buf.data(), bytes);
  return true;
}

static void write_u32(std::FILE* f, const uint32_t* a, uint64_t count) {
  if (count) std::fwrite(a, 4, count, f);
  if (count & 1u) {
    const uint32_t pad = 0;
    std::fwrite(&pad, 4, 1, f);
  }
}

// What a map owns (dmap.hpp Store), each array its own block.
struct Map {
  uint64_t max_keys, cap, seed;
  bool force_home;
  uint64_t force_at;
  uint32_t *table, *scope, *count;
  uint8_t* digests;
  uint64_t head[dm::kHeadWords];
  Map(uint64_t max_keys_, uint64_t seed_, int64_t home)
      : max_keys(max_keys_), cap(dm::capacity(max_keys_)), seed(seed_), force_home(home >= 0),
        force_at(home >= 0 ? (uint64_t)home : 0), table(exact<uint32_t>(cap)), scope(exact_filled<uint32_t>(max_keys_, kSentinel)),
        count(exact_filled<uint32_t>(max_keys_, kSentinel)), digests(exact_filled<uint8_t>(32 * max_keys_, 0xA5)) {
    clear();
  }
  ~Map() {
    std::free(table);
    std::free(scope);
    std::free(count);
    std::free(digests);
  }
  Map(const Map&) = delete;
  Map& operator=(const Map&) = delete;
  void clear() {  // k_dmap_clear
    for (uint64_t p = 0; p < cap; ++p) table[p] = dm::kEmpty;
    for (uint32_t w = 0; w < dm::kHeadWords; ++w) head[w] = 0;
  }
  gp::Placement placement() const {
    gp::Placement pl;
    pl.seed = seed;
    pl.mask = (uint32_t)(cap - 1);
    pl.force_home = force_home ? 1u : 0u;
    pl.force_at = (uint32_t)(force_at % cap);
    return pl;
  }
  gp::Key stored(uint32_t e) const {
    gp::Key k;
    k.scope = scope[e];
    std::memcpy(k.lo.d, digests + 32ull * e, 16);
    std::memcpy(k.hi.d, digests + 32ull * e + 16, 16);
    return k;
  }
  // every byte a refused call must leave alone
  std::vector<uint8_t> bytes() const {
    std::vector<uint8_t> b(4 * cap + 36 * max_keys + 4 * max_keys + 8);
    uint8_t* p = b.data();
    std::memcpy(p, table, 4 * cap), p += 4 * cap;
    std::memcpy(p, scope, 4 * max_keys), p += 4 * max_keys;
    std::memcpy(p, digests, 32 * max_keys), p += 32 * max_keys;
    std::memcpy(p, count, 4 * max_keys), p += 4 * max_keys;
    std::memcpy(p, &head[dm::kHeadEntries], 8);
    return b;
  }
  // the table holds each id below entries exactly once and nothing else, and is half empty
  void check_table() const {
    const uint64_t entries = head[dm::kHeadEntries];
    CHECK(entries <= max_keys && 2 * entries <= cap, "entries %llu of %llu", (ull)entries, (ull)max_keys);
    std::vector<uint8_t> seen(entries, 0);
    for (uint64_t p = 0; p < cap; ++p) {
      if (table[p] == dm::kEmpty) continue;
      CHECK(table[p] < entries && !seen[table[p]], "position %llu holds %u", (ull)p, table[p]);
      if (table[p] < entries) seen[table[p]] = 1;
    }
    for (uint64_t e = 0; e < entries; ++e) CHECK(seen[e], "id %llu is not in the table", (ull)e);
  }
};

struct Inputs {
  uint64_t n = 0, crossed_cap = 0;
  uint32_t threshold = 0;
  bool counts = true;
  const uint8_t* digests = nullptr;
  const uint32_t* scope = nullptr;
};

static gp::Key key_of(const Inputs& in, uint64_t s) {
  gp::Key k;
  k.scope = in.scope ? in.scope[s] : 0u;
  std::memcpy(k.lo.d, in.digests + 32 * s, 16);
  std::memcpy(k.hi.d, in.digests + 32 * s + 16, 16);
  return k;
}

struct Outputs {
  uint32_t *id, *before, *after, *crossed;  // before doubles as find's count
  uint64_t r[8];
  Outputs(const Inputs& in)
      : id(exact_filled<uint32_t>(in.n, kSentinel)), before(in.counts ? exact_filled<uint32_t>(in.n, kSentinel) : nullptr),
        after(in.counts ? exact_filled<uint32_t>(in.n, kSentinel) : nullptr),
        crossed(exact_filled<uint32_t>(in.crossed_cap, kSentinel)) {
    std::memset(r, 0xFF, sizeof r);
  }
  ~Outputs() {
    std::free(id);
    std::free(before);
    std::free(after);
    std::free(crossed);
  }
  Outputs(const Outputs&) = delete;
  Outputs& operator=(const Outputs&) = delete;
};

// One workgroup's scan of `totals` (k_dmap_scan's use of group::scan_walk): every thread's
// walk, the workgroup prefix of each chunk worked out beforehand. Returns the sum.
static uint64_t scan(uint32_t* totals, uint64_t tiles) {
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
  uint64_t total = 0;
  for (uint32_t t = 0; t < gp::kScanThreads; ++t) {
    uint64_t chunk = 0;
    const uint64_t g = gp::scan_walk(
        tiles, t, [&](uint64_t k) { return totals[k]; },
        [&](uint32_t, uint32_t* bf, uint32_t* al) {
          *bf = before[chunk * gp::kScanThreads + t];
          *al = all[chunk];
          ++chunk;
        },
        [&](uint64_t k, uint32_t b) {
          totals[k] = b;
          stored[k]++;
        });
    if (t == 0) total = g;
    CHECK(g == total, "thread %u sums %llu, thread 0 %llu", t, (ull)g, (ull)total);
  }
  for (uint64_t k = 0; k < tiles; ++k) CHECK(stored[k] == 1, "tile base %llu stored %d times", (ull)k, stored[k]);
  return total;
}

// A read-only walk for key k: dmap::find_probe.
static dm::Found walk(const Map& m, const gp::Key& k) {
  const gp::Placement pl = m.placement();
  uint64_t steps = 0;
  const dm::Found f = dm::find_probe(
      gp::home(pl, k), pl.mask,
      [&](uint32_t p) {
        ++steps;
        return m.table[p];
      },
      [&](uint32_t e) {
        CHECK(e < m.head[dm::kHeadEntries], "the table holds id %u of %llu", e, (ull)m.head[dm::kHeadEntries]);
        return e < m.max_keys && gp::same(k, m.stored(e));
      });
  CHECK(steps <= m.cap, "a walk of %llu steps", (ull)steps);
  return f;
}

// The seven kernels of one add, the lanes of the call's insert and of commit in `order`.
static void run_add(Map* m, const Inputs& in, const std::vector<uint32_t>& order, Outputs* out) {
  const uint64_t n = in.n;
  const dm::CallLayout lay(n);
  const uint64_t tiles = gp::tiles(n);
  uint32_t* const table = exact_filled<uint32_t>(lay.g.cap, gp::kEmpty);  // k_group_init
  uint32_t* const pos = exact_filled<uint32_t>(n, kSentinel);
  uint32_t* const first = exact_filled<uint32_t>(n, kSentinel);
  uint32_t* const members = exact_filled<uint32_t>(n, 0u);
  uint32_t* const lead_id = exact_filled<uint32_t>(n, kSentinel);
  uint32_t* const lead_pos = exact_filled<uint32_t>(n, kSentinel);
  uint32_t* const lead_before = exact_filled<uint32_t>(n, kSentinel);
  uint32_t* const tot_new = exact<uint32_t>(tiles);
  uint32_t* const tot_cross = exact<uint32_t>(tiles);
  uint64_t best = 0;

  // k_group_insert and k_group_resolve (tests/cpp/group_check.cpp checks them in full)
  gp::Placement pl;
  pl.seed = kCallSeed;
  pl.mask = (uint32_t)(lay.g.cap - 1);
  for (uint32_t i : order) {
    const gp::Key k = key_of(in, i);
    pos[i] = gp::probe(
        i, gp::home(pl, k), pl.mask, [&](uint32_t p) { return table[p]; },
        [&](uint32_t p, uint32_t me) {
          const uint32_t old = table[p];
          if (old == gp::kEmpty) table[p] = me;
          return old;
        },
        [&](uint32_t p, uint32_t me) {
          if (me < table[p]) table[p] = me;
        },
        [&](uint32_t j) { return j < n && gp::same(k, key_of(in, j)); });
  }
  for (uint64_t i = 0; i < n; ++i) {
    first[i] = table[pos[i]];
    CHECK(first[i] <= i, "slot %llu follows %u", (ull)i, first[i]);
    members[first[i]]++;
  }
  const auto leads = [&](uint64_t i) { return i < n && first[i] == i; };

  // k_dmap_find: leaders only, the map read-only
  const std::vector<uint8_t> untouched = m->bytes();
  for (uint64_t tile = 0; tile < tiles; ++tile) {
    uint32_t fresh = 0, crossing = 0;
    for (uint64_t i = tile * dm::kTile; i < n && i < (tile + 1) * dm::kTile; ++i) {
      if (!leads(i)) continue;
      const dm::Found f = walk(*m, key_of(in, i));
      const bool is_new = f.id == dm::kNew;
      const uint32_t before = is_new ? 0u : m->count[f.id];
      lead_id[i] = f.id;
      lead_pos[i] = f.pos;
      lead_before[i] = before;
      fresh += is_new;
      crossing += dm::crossed(in.threshold, before, dm::sat_add(before, members[i]));
    }
    tot_new[tile] = fresh;
    tot_cross[tile] = crossing;
  }

  // k_dmap_scan
  const uint64_t entries_before = m->head[dm::kHeadEntries];
  m->head[dm::kHeadAdded] = scan(tot_new, tiles);
  m->head[dm::kHeadCrossed] = scan(tot_cross, tiles);
  const bool full = dm::refuse(entries_before, m->head[dm::kHeadAdded], m->max_keys);
  m->head[dm::kHeadFull] = full;

  // k_dmap_commit: nothing when full
  if (!full) {
    std::vector<uint8_t> listed(in.crossed_cap, 0);
    // what every lane loads before its tile's barrier: commit writes lead_id behind it
    std::vector<uint8_t> was_new(n, 0);
    for (uint64_t i = 0; i < n; ++i) was_new[i] = leads(i) && lead_id[i] == dm::kNew;
    for (uint32_t i : order) {
      if (!leads(i)) continue;
      const uint64_t tile = i / dm::kTile;
      const uint32_t t = i % dm::kTile;
      uint64_t b_new[dm::kTileWaves] = {}, b_cross[dm::kTileWaves] = {};
      for (uint32_t u = 0; u < dm::kTile; ++u) {
        const uint64_t j = tile * dm::kTile + u;
        if (!leads(j)) continue;
        if (was_new[j])
          b_new[u >> 6] |= uint64_t(1) << (u & 63u);
        if (dm::crossed(in.threshold, lead_before[j], dm::sat_add(lead_before[j], members[j])))
          b_cross[u >> 6] |= uint64_t(1) << (u & 63u);
      }
      const bool is_new = (b_new[t >> 6] >> (t & 63u)) & 1u;
      const uint32_t after = dm::sat_add(lead_before[i], members[i]);
      uint32_t id = lead_id[i];
      if (is_new) {
        id = dm::new_id(entries_before, (uint64_t)tot_new[tile] + gp::rank_in_tile(b_new, t >> 6, t & 63u));
        CHECK(id < m->max_keys, "id %u of %llu", id, (ull)m->max_keys);
        const gp::Key k = key_of(in, i);
        m->scope[id] = k.scope;
        std::memcpy(m->digests + 32ull * id, k.lo.d, 16);
        std::memcpy(m->digests + 32ull * id + 16, k.hi.d, 16);
        lead_id[i] = id;
        uint64_t steps = 0;
        dm::insert_probe(id, lead_pos[i], (uint32_t)(m->cap - 1), [&](uint32_t p, uint32_t me) {
          ++steps;
          const uint32_t old = m->table[p];
          if (old == dm::kEmpty) m->table[p] = me;
          return old;
        });
        CHECK(steps <= m->cap, "an insert of %llu steps", (ull)steps);
      }
      m->count[id] = after;
      if ((b_cross[t >> 6] >> (t & 63u)) & 1u) {
        const uint64_t r = (uint64_t)tot_cross[tile] + gp::rank_in_tile(b_cross, t >> 6, t & 63u);
        if (r < in.crossed_cap) {
          CHECK(!listed[r], "crossed entry %llu written twice", (ull)r);
          listed[r] = 1;
          out->crossed[r] = i;
        }
      }
      const uint64_t key = gp::best_key(after, id);
      best = key > best ? key : best;
    }
  } else {
    CHECK(m->bytes() == untouched, "a refused call changed the map");
  }

  // k_dmap_fill
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t f = first[i];
    out->id[i] = full ? dm::kNoId : lead_id[f];
    if (out->before) out->before[i] = lead_before[f];
    if (out->after) out->after[i] = dm::sat_add(lead_before[f], members[f]);
  }
  dm::result_words(n, entries_before, m->head[dm::kHeadAdded], full, m->head[dm::kHeadCrossed], in.crossed_cap, best, out->r);
  m->head[dm::kHeadEntries] = out->r[1];
  if (full) CHECK(m->bytes() == untouched, "a refused call changed the map");
  m->check_table();

  std::free(table);
  std::free(pos);
  std::free(first);
  std::free(members);
  std::free(lead_id);
  std::free(lead_pos);
  std::free(lead_before);
  std::free(tot_new);
  std::free(tot_cross);
}

// k_dmap_lookup
static void run_find(const Map& m, const Inputs& in, Outputs* out) {
  const std::vector<uint8_t> untouched = m.bytes();
  for (uint64_t i = 0; i < in.n; ++i) {
    const dm::Found f = walk(m, key_of(in, i));
    const bool found = f.id != dm::kNew;
    out->id[i] = found ? f.id : dm::kNoId;
    if (out->before) out->before[i] = found ? m.count[f.id] : 0u;
  }
  CHECK(m.bytes() == untouched, "a find changed the map");
}

static bool same_u32(const uint32_t* a, const uint32_t* b, uint64_t count) {
  return (!a && !b) || count == 0 || (a && b && std::memcmp(a, b, 4 * count) == 0);
}

// what msha_dmap_read returns for all entries
static bool same_state(const Map& a, const Map& b) {
  const uint64_t e = a.head[dm::kHeadEntries];
  return e == b.head[dm::kHeadEntries] &&
         (e == 0 || (std::memcmp(a.scope, b.scope, 4 * e) == 0 && std::memcmp(a.digests, b.digests, 32 * e) == 0 &&
                     std::memcmp(a.count, b.count, 4 * e) == 0));
}

static void check_units() {
  CHECK(dm::sat_add(0, 0) == 0 && dm::sat_add(5, 7) == 12, "sat_add");
  CHECK(dm::sat_add(0xFFFFFFFEu, 1) == 0xFFFFFFFFu && dm::sat_add(0xFFFFFFFEu, 2) == 0xFFFFFFFFu, "sat_add at the top");
  CHECK(dm::sat_add(0xFFFFFFFFu, 0x40000000u) == 0xFFFFFFFFu && dm::sat_add(0xC0000000u, 0x40000000u) == 0xFFFFFFFFu,
        "sat_add saturates");
  CHECK(dm::sat_add(0xBFFFFFFFu, 0x40000000u) == 0xFFFFFFFFu && dm::sat_add(0xBFFFFFFEu, 0x40000000u) == 0xFFFFFFFEu,
        "sat_add below the top");
  CHECK(dm::crossed(3, 0, 3) && dm::crossed(3, 2, 3) && dm::crossed(3, 2, 9), "crossed");
  CHECK(!dm::crossed(3, 3, 5) && !dm::crossed(3, 1, 2) && !dm::crossed(0, 0, 5) && !dm::crossed(3, 3, 3), "not crossed");
  CHECK(dm::crossed(0xFFFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFFFu) && !dm::crossed(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu),
        "crossed at the top");
  CHECK(!dm::refuse(0, 4, 4) && dm::refuse(0, 5, 4) && dm::refuse(3, 2, 4) && !dm::refuse(3, 1, 4) && !dm::refuse(4, 0, 4),
        "refuse");
  CHECK(!dm::refuse(dm::kMaxKeys - 1, 1, dm::kMaxKeys) && dm::refuse(dm::kMaxKeys, dm::kMaxSlots, dm::kMaxKeys), "refuse at the top");
  CHECK(dm::new_id(0, 0) == 0 && dm::new_id(7, 3) == 10, "new_id");
  uint64_t r[8];
  dm::result_words(9, 4, 2, false, 5, 3, gp::best_key(6, 1), r);
  const uint64_t ok[8] = {9, 6, 2, 0, 5, 3, 6, 1};
  CHECK(std::memcmp(r, ok, sizeof r) == 0, "result_words");
  dm::result_words(9, 4, 2, true, 5, 3, 0, r);
  const uint64_t refused[8] = {9, 4, 2, 1, 0, 0, 0, 0};
  CHECK(std::memcmp(r, refused, sizeof r) == 0, "result_words of a refused call");
  dm::result_words(1, 0, 1, false, 0, 0, gp::best_key(0xFFFFFFFFu, 0), r);
  CHECK(r[6] == 0xFFFFFFFFull && r[7] == 0 && r[5] == 0, "result_words at the top");

  // capacity a power of two, at least 2 max_keys and one wave's worth; the arrays in
  // order, each 256-aligned and large enough, none overlapping the next
  std::vector<uint64_t> ks = {1, 2, 3, 4, 8, 31, 32, 33, 63, 64, 65, 300, 4097};
  for (uint32_t b = 7; b <= 30; ++b) {
    ks.push_back((uint64_t(1) << b) - 1);
    ks.push_back(uint64_t(1) << b);
    if (b < 30) ks.push_back((uint64_t(1) << b) + 1);
  }
  for (uint64_t k : ks) {
    const dm::Store lay(k);
    CHECK(lay.cap == dm::capacity(k) && (lay.cap & (lay.cap - 1)) == 0 && lay.cap >= 2 * k && lay.cap >= 64 &&
              lay.cap <= (uint64_t(1) << 31) && (lay.cap == 64 || lay.cap < 4 * k),
          "max_keys %llu: capacity %llu", (ull)k, (ull)lay.cap);
    const uint64_t at[6] = {lay.head, lay.table, lay.scope, lay.digests, lay.count, lay.bytes};
    const uint64_t need[5] = {8 * dm::kHeadWords, 4 * lay.cap, 4 * k, 32 * k, 4 * k};
    for (uint32_t j = 0; j < 5; ++j)
      CHECK(at[j] % 256 == 0 && at[j] + need[j] <= at[j + 1], "max_keys %llu: array %u", (ull)k, j);
    const dm::CallLayout c(k);  // k as a slot count
    const uint64_t cat[6] = {c.first, c.ppos, c.before, c.tot_new, c.tot_cross, c.bytes};
    const uint64_t cneed[5] = {4 * k, 4 * k, 4 * k, 4 * gp::tiles(k), 4 * gp::tiles(k)};
    CHECK(c.first == c.g.bytes, "n %llu: the call's arrays start behind group's", (ull)k);
    for (uint32_t j = 0; j < 5; ++j)
      CHECK(cat[j] % 256 == 0 && cat[j] + cneed[j] <= cat[j + 1], "n %llu: call array %u", (ull)k, j);
  }
  CHECK(dm::capacity(8) == 64 && dm::capacity(32) == 64 && dm::capacity(33) == 128 && dm::capacity(dm::kMaxKeys) == uint64_t(1) << 31,
        "capacity");
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::printf("usage: dmap_check SEQUENCES RESULTS\n");
    return 2;
  }
  std::FILE* in_f = std::fopen(argv[1], "rb");
  std::FILE* out_f = std::fopen(argv[2], "wb");
  int64_t count = 0;
  if (!in_f || !out_f || std::fread(&count, 8, 1, in_f) != 1) {
    std::printf("cannot open the sequence or the result file\n");
    return 2;
  }
  g_seq = g_step = ~uint64_t(0);
  check_units();
  std::printf("units and layout checked\n");

  uint64_t steps_run = 0;
  for (int64_t q = 0; q < count; ++q) {
    g_seq = (uint64_t)q;
    g_step = ~uint64_t(0);
    int64_t sh[3];
    if (std::fread(sh, 8, 3, in_f) != 3) return 2;
    // three maps, three seeds: where a key lies differs between them as well
    Map m0((uint64_t)sh[0], 0x1111111111111111ull, sh[1]), m1((uint64_t)sh[0], 0xFEDCBA9876543210ull, sh[1]),
        m2((uint64_t)sh[0], 0x0F0F0F0F0F0F0F0Full + (uint64_t)q, sh[1]);
    for (int64_t s = 0; s < sh[2]; ++s, ++steps_run) {
      g_step = (uint64_t)s;
      int64_t h[7];
      if (std::fread(h, 8, 7, in_f) != 7) return 2;
      const int kind = (int)h[0];
      const uint64_t n = (uint64_t)h[1], n_flips = (uint64_t)h[5];
      Inputs in;
      in.n = n;
      in.threshold = (uint32_t)h[3];
      in.crossed_cap = (uint64_t)h[4];
      in.counts = h[6] != 0;
      uint8_t* digests = nullptr;
      uint32_t* scope = nullptr;
      if (kind != kClear) {
        std::vector<uint32_t> val(n), flips(2 * n_flips);
        if (!read_words(in_f, val.data(), 4 * n)) return 2;
        if (h[2]) {
          scope = exact<uint32_t>(n);
          if (!read_words(in_f, scope, 4 * n)) return 2;
        }
        if (!read_words(in_f, flips.data(), 8 * n_flips)) return 2;
        digests = exact<uint8_t>(32 * n);
        for (uint64_t i = 0; i < n; ++i) base_row(val[i], digests + 32 * i);
        for (uint64_t j = 0; j < n_flips; ++j) digests[32ull * flips[2 * j] + flips[2 * j + 1]] ^= kFlip;
      }
      in.digests = digests;
      in.scope = scope;

      // ascending, descending, and a Fisher-Yates shuffle driven by a fixed LCG
      std::vector<uint32_t> up(n), down(n), mixed(n);
      for (uint64_t i = 0; i < n; ++i) {
        up[i] = mixed[i] = (uint32_t)i;
        down[i] = (uint32_t)(n - 1 - i);
      }
      uint64_t lcg = 0x2545F4914F6CDD1Dull + (uint64_t)q * 131 + (uint64_t)s;
      for (uint64_t i = n; i > 1; --i) {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        const uint64_t j = (lcg >> 33) % i;
        std::swap(mixed[i - 1], mixed[j]);
      }

      Outputs a(in), b(in), c(in);
      if (kind == kAdd) {
        run_add(&m0, in, up, &a);
        run_add(&m1, in, down, &b);
        run_add(&m2, in, mixed, &c);
      } else if (kind == kFind) {
        run_find(m0, in, &a);
        run_find(m1, in, &b);
        run_find(m2, in, &c);
      } else {
        m0.clear();
        m1.clear();
        m2.clear();
      }
      for (const Outputs* o : {&b, &c}) {
        CHECK(same_u32(a.id, o->id, n) && same_u32(a.before, o->before, n) && same_u32(a.after, o->after, n) &&
                  same_u32(a.crossed, o->crossed, in.crossed_cap) && std::memcmp(a.r, o->r, sizeof a.r) == 0,
              "another lane order or seed gives another answer");
      }
      CHECK(same_state(m0, m1) && same_state(m0, m2), "another lane order or seed leaves another map");

      const std::vector<uint32_t> unset(n, kSentinel);
      if (kind == kAdd) {
        std::fwrite(a.r, 8, 8, out_f);
        write_u32(out_f, a.id, n);
        write_u32(out_f, a.before ? a.before : unset.data(), n);
        write_u32(out_f, a.after ? a.after : unset.data(), n);
        write_u32(out_f, a.crossed, in.crossed_cap);
      } else if (kind == kFind) {
        write_u32(out_f, a.id, n);
        write_u32(out_f, a.before ? a.before : unset.data(), n);
      }
      const uint64_t entries = m0.head[dm::kHeadEntries];
      std::fwrite(&entries, 8, 1, out_f);
      write_u32(out_f, m0.scope, entries);
      if (entries) std::fwrite(m0.digests, 32, entries, out_f);
      write_u32(out_f, m0.count, entries);
      std::free(scope);
      std::free(digests);
    }
  }
  std::fclose(in_f);
  std::fclose(out_f);
  if (g_failed) {
    std::printf("dmap FAILED: %d checks\n", g_failed);
    return 1;
  }
  std::printf("dmap ok: %lld sequences, %llu steps\n", (long long)count, (ull)steps_run);
  return 0;
}
