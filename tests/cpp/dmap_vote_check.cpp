// Stand-alone check of mirbft_amd/csrc/dmap_vote.hpp (tests/test_dmap_vote_cpu.py builds it
// with -fsanitize=address,undefined and runs it). The header is what the kernels of a vote
// map run; here the lanes run one after the other, and plain loads and stores stand in for
// the atomic load, the compare-and-swap, the min, the add and the or.
//
// Every array is a heap block of exactly its contract size: of the caller's, 32 n bytes of
// digests, 4 n of scopes and of voters, n entries each of id, counted, before and after,
// crossed_cap entries of the crossed list; of the map, capacity(max_keys) table entries,
// max_keys scopes, 32 max_keys digest bytes, max_keys counts and max_keys * words mask
// words; of the call's workspace, n entries each of first, the leaders' id, position and
// before, the pair positions, counted and fresh, capacity(n) entries of each table and
// tiles(n) totals five times. So a mask word past max_keys * words, a pair position past
// the pair table's capacity or a stored key past max_keys is an AddressSanitizer report.
//
// Each sequence runs on three maps: the lanes of the call's insert, of the PAIR INSERT, of
// the commit and of the fill's mask writes go in ascending, descending and a fixed
// shuffled order, under three seeds. After every step every output and everything
// msha_dmap_read and msha_dmap_read_voters would return must be the same on all three, and
// count[id] == popcount(mask[id]) must hold. A refused vote must leave every byte of the
// map as it was. The first map's outputs go to the result file, which the pytest file
// compares with its dict-of-sets oracle.
//
// argv[1]: the sequences tests/dmap_vote_matrix.py wrote (write_sequences); argv[2]: where
// the results go (read_results).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mirbft_amd/csrc/dmap_vote.hpp"

namespace gp = msha::group;
namespace dm = msha::dmap;
namespace dv = msha::dmap_vote;

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
enum { kClear = 2, kVote = 3, kFindVotes = 4 };

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

// What a vote map owns (dmap_vote.hpp VoteStore), each array its own block.
struct Map {
  uint64_t max_keys, cap, seed;
  uint32_t max_voters, words;
  bool force_home;
  uint64_t force_at;
  uint32_t *table, *scope, *count, *masks;
  uint8_t* digests;
  uint64_t head[dm::kHeadWords];
  Map(uint64_t max_keys_, uint32_t max_voters_, uint64_t seed_, int64_t home)
      : max_keys(max_keys_), cap(dm::capacity(max_keys_)), seed(seed_), max_voters(max_voters_), words(dv::words(max_voters_)),
        force_home(home >= 0), force_at(home >= 0 ? (uint64_t)home : 0), table(exact<uint32_t>(cap)),
        scope(exact_filled<uint32_t>(max_keys_, kSentinel)), count(exact_filled<uint32_t>(max_keys_, kSentinel)),
        masks(exact_filled<uint32_t>(max_keys_ * words, kSentinel)), digests(exact_filled<uint8_t>(32 * max_keys_, 0xA5)) {
    clear();
  }
  ~Map() {
    std::free(table);
    std::free(scope);
    std::free(count);
    std::free(masks);
    std::free(digests);
  }
  Map(const Map&) = delete;
  Map& operator=(const Map&) = delete;
  void clear() {  // k_dmap_clear on a vote map: the masks as well (dmap_vote.hpp "mask")
    for (uint64_t p = 0; p < cap; ++p) table[p] = dm::kEmpty;
    for (uint32_t w = 0; w < dm::kHeadWords; ++w) head[w] = 0;
    for (uint64_t q = 0; q < max_keys * words; ++q) masks[q] = 0;
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
  uint32_t& mask_at(uint32_t id, uint32_t voter) { return masks[(uint64_t)id * words + dv::mask_word(voter)]; }
  // every byte a refused call must leave alone
  std::vector<uint8_t> bytes() const {
    std::vector<uint8_t> b(4 * cap + 40 * max_keys + 4 * max_keys * words + 8);
    uint8_t* p = b.data();
    std::memcpy(p, table, 4 * cap), p += 4 * cap;
    std::memcpy(p, scope, 4 * max_keys), p += 4 * max_keys;
    std::memcpy(p, digests, 32 * max_keys), p += 32 * max_keys;
    std::memcpy(p, count, 4 * max_keys), p += 4 * max_keys;
    std::memcpy(p, masks, 4 * max_keys * words), p += 4 * max_keys * words;
    std::memcpy(p, &head[dm::kHeadEntries], 8);
    return b;
  }
  // the table holds each id below entries once and nothing else; count is popcount(mask),
  // no bit at or past max_voters is set, and the masks past entries are empty
  void check() const {
    const uint64_t entries = head[dm::kHeadEntries];
    CHECK(entries <= max_keys && 2 * entries <= cap, "entries %llu of %llu", (ull)entries, (ull)max_keys);
    std::vector<uint8_t> seen(entries, 0);
    for (uint64_t p = 0; p < cap; ++p) {
      if (table[p] == dm::kEmpty) continue;
      CHECK(table[p] < entries && !seen[table[p]], "position %llu holds %u", (ull)p, table[p]);
      if (table[p] < entries) seen[table[p]] = 1;
    }
    for (uint64_t e = 0; e < max_keys; ++e) {
      uint32_t bits = 0;
      for (uint32_t w = 0; w < words; ++w) {
        const uint32_t m = masks[e * words + w];
        bits += (uint32_t)__builtin_popcount(m);
        const uint32_t valid = max_voters >= 32 * (w + 1) ? 0xFFFFFFFFu : (1u << (max_voters - 32 * w)) - 1u;
        CHECK((m & ~valid) == 0, "id %llu word %u has a bit past max_voters: %08x", (ull)e, w, m);
      }
      if (e < entries) {
        CHECK(seen[e], "id %llu is not in the table", (ull)e);
        CHECK(bits == count[e], "id %llu: count %u, popcount(mask) %u", (ull)e, count[e], bits);
      } else {
        CHECK(bits == 0, "id %llu is not given out and its mask is not empty", (ull)e);
      }
    }
  }
};

struct Inputs {
  uint64_t n = 0, crossed_cap = 0;
  uint32_t threshold = 0;
  bool counts = true;
  const uint8_t* digests = nullptr;
  const uint32_t* scope = nullptr;
  const uint32_t* voter = nullptr;
  int64_t pair_home = -1;
};

static gp::Key key_of(const Inputs& in, uint64_t s) {
  gp::Key k;
  k.scope = in.scope ? in.scope[s] : 0u;
  std::memcpy(k.lo.d, in.digests + 32 * s, 16);
  std::memcpy(k.hi.d, in.digests + 32 * s + 16, 16);
  return k;
}

struct Outputs {
  uint32_t *id, *counted, *before, *after, *crossed, *voted;  // before doubles as find_votes' count
  uint64_t r[dv::kResultWords];
  Outputs(const Inputs& in, bool find)
      : id(exact_filled<uint32_t>(in.n, kSentinel)), counted(in.counts && !find ? exact_filled<uint32_t>(in.n, kSentinel) : nullptr),
        before(in.counts ? exact_filled<uint32_t>(in.n, kSentinel) : nullptr),
        after(in.counts && !find ? exact_filled<uint32_t>(in.n, kSentinel) : nullptr),
        crossed(exact_filled<uint32_t>(in.crossed_cap, kSentinel)), voted(find ? exact_filled<uint32_t>(in.n, kSentinel) : nullptr) {
    std::memset(r, 0xFF, sizeof r);
  }
  ~Outputs() {
    std::free(id);
    std::free(counted);
    std::free(before);
    std::free(after);
    std::free(crossed);
    std::free(voted);
  }
  Outputs(const Outputs&) = delete;
  Outputs& operator=(const Outputs&) = delete;
};

// One workgroup's scan of `totals` (k_vote_scan's use of group::scan_walk): every thread's
// walk, the workgroup prefix of each chunk worked out beforehand. keep: the bases are
// stored (the two totals that rank), else the sum alone is wanted. Returns the sum.
static uint64_t scan(uint32_t* totals, uint64_t tiles, bool keep) {
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
  std::vector<uint32_t> bases(tiles, 0);
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
          bases[k] = b;  // a thread stores its own tile alone: no later load sees a base
          stored[k]++;
        });
    if (t == 0) total = g;
    CHECK(g == total, "thread %u sums %llu, thread 0 %llu", t, (ull)g, (ull)total);
  }
  for (uint64_t k = 0; k < tiles; ++k) {
    CHECK(stored[k] == 1, "tile base %llu stored %d times", (ull)k, stored[k]);
    if (keep) totals[k] = bases[k];
  }
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

// The ten kernels of one vote, the lanes of both inserts, of commit and of fill in `order`.
static void run_vote(Map* m, const Inputs& in, const std::vector<uint32_t>& order, uint64_t call_seed, Outputs* out) {
  const uint64_t n = in.n;
  const dv::VoteLayout lay(n);
  const uint64_t tiles = gp::tiles(n);
  uint32_t* const table = exact_filled<uint32_t>(lay.c.g.cap, gp::kEmpty);  // k_group_init
  uint32_t* const pos = exact_filled<uint32_t>(n, kSentinel);
  uint32_t* const first = exact_filled<uint32_t>(n, kSentinel);
  uint32_t* const lead_id = exact_filled<uint32_t>(n, kSentinel);
  uint32_t* const lead_pos = exact_filled<uint32_t>(n, kSentinel);
  uint32_t* const lead_before = exact_filled<uint32_t>(n, kSentinel);
  uint32_t* const pair_table = exact_filled<uint32_t>(lay.pair_cap, kSentinel - 1);  // k_vote_find empties it
  uint32_t* const pair_pos = exact_filled<uint32_t>(n, kSentinel);
  uint32_t* const counted = exact_filled<uint32_t>(n, kSentinel);
  uint32_t* const fresh = exact_filled<uint32_t>(n, kSentinel);
  uint32_t* const tot_new = exact<uint32_t>(tiles);
  uint32_t* const tot_cross = exact<uint32_t>(tiles);
  uint32_t* const tot_counted = exact<uint32_t>(tiles);
  uint32_t* const tot_repeats = exact<uint32_t>(tiles);
  uint32_t* const tot_bad = exact<uint32_t>(tiles);
  uint64_t best = 0;

  // k_group_insert and k_group_resolve (tests/cpp/group_check.cpp checks them in full)
  gp::Placement pl;
  pl.seed = call_seed;
  pl.mask = (uint32_t)(lay.c.g.cap - 1);
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
  }
  const auto leads = [&](uint64_t i) { return i < n && first[i] == i; };

  // k_vote_find: the pair table and fresh cleared by the grid's threads, four entries
  // each; leaders walk the map read-only
  const std::vector<uint8_t> untouched = m->bytes();
  const uint64_t threads = tiles * dm::kTile;
  CHECK(lay.pair_cap % 4 == 0 && lay.pair_cap / 4 <= threads && (n + 3) / 4 <= threads, "the grid of %llu threads clears both",
        (ull)threads);
  for (uint64_t q = 0; q < lay.pair_cap / 4; ++q)
    for (uint32_t j = 0; j < 4; ++j) pair_table[4 * q + j] = gp::kEmpty;
  CHECK(4 * ((n + 3) / 4) <= msha::round256(4 * n) / 4, "fresh's quads stay inside its 256-byte pieces");
  for (uint64_t i = 0; i < n; ++i) fresh[i] = 0;  // (the block here is n entries, the workspace's whole 256 bytes)
  for (uint64_t i = 0; i < n; ++i) {
    if (!leads(i)) continue;
    const dm::Found f = walk(*m, key_of(in, i));
    lead_id[i] = f.id;
    lead_pos[i] = f.pos;
    lead_before[i] = f.id == dm::kNew ? 0u : m->count[f.id];
  }

  // k_vote_pair: slots with a voter in range, in `order`
  gp::Placement pp;
  pp.seed = call_seed;
  pp.mask = (uint32_t)(lay.pair_cap - 1);
  pp.force_home = in.pair_home >= 0 ? 1u : 0u;
  pp.force_at = in.pair_home >= 0 ? (uint32_t)((uint64_t)in.pair_home % lay.pair_cap) : 0u;
  for (uint32_t i : order) {
    const uint32_t v = in.voter[i];
    if (!dv::in_range(v, m->max_voters)) continue;
    const uint32_t f = first[i];
    uint64_t steps = 0;
    pair_pos[i] = gp::probe(
        i, gp::home_of(pp, dv::pair_hash(pp.seed, f, v)), pp.mask,
        [&](uint32_t p) {
          ++steps;
          return pair_table[p];
        },
        [&](uint32_t p, uint32_t me) {
          const uint32_t old = pair_table[p];
          if (old == gp::kEmpty) pair_table[p] = me;
          return old;
        },
        [&](uint32_t p, uint32_t me) {
          if (me < pair_table[p]) pair_table[p] = me;
        },
        [&](uint32_t j) {
          CHECK(j < n && dv::in_range(in.voter[j < n ? j : 0], m->max_voters), "the pair table holds slot %u", j);
          return j < n && dv::pair_same(f, v, first[j], in.voter[j]);
        });
    CHECK(steps <= lay.pair_cap, "a pair insert of %llu steps", (ull)steps);
  }

  // k_vote_count
  for (uint64_t tile = 0; tile < tiles; ++tile) {
    uint32_t c = 0, r = 0, b = 0;
    for (uint64_t i = tile * dm::kTile; i < n && i < (tile + 1) * dm::kTile; ++i) {
      const uint32_t v = in.voter[i];
      bool counts = false;
      if (dv::in_range(v, m->max_voters)) {
        const bool pair_leader = pair_table[pair_pos[i]] == i;
        uint32_t word = 0;
        if (pair_leader) {
          const uint32_t id = lead_id[first[i]];
          if (id != dm::kNew) word = m->mask_at(id, v);
        }
        counts = dv::counted(pair_leader, word, v);
        r += !counts;
      } else {
        ++b;
      }
      counted[i] = counts;
      c += counts;
      if (counts) fresh[first[i]]++;
    }
    tot_counted[tile] = c;
    tot_repeats[tile] = r;
    tot_bad[tile] = b;
  }

  // k_vote_totals
  const auto after_of = [&](uint64_t i) { return lead_before[i] + fresh[i]; };
  for (uint64_t tile = 0; tile < tiles; ++tile) {
    uint32_t fresh_keys = 0, crossing = 0;
    for (uint64_t i = tile * dm::kTile; i < n && i < (tile + 1) * dm::kTile; ++i) {
      if (!leads(i)) continue;
      CHECK(after_of(i) <= m->max_voters, "slot %llu: a count of %u", (ull)i, after_of(i));
      fresh_keys += lead_id[i] == dm::kNew;
      crossing += dm::crossed(in.threshold, lead_before[i], after_of(i));
    }
    tot_new[tile] = fresh_keys;
    tot_cross[tile] = crossing;
  }

  // k_vote_scan
  const uint64_t entries_before = m->head[dm::kHeadEntries];
  m->head[dm::kHeadAdded] = scan(tot_new, tiles, true);
  m->head[dm::kHeadCrossed] = scan(tot_cross, tiles, true);
  const uint64_t n_counted = scan(tot_counted, tiles, false), n_repeats = scan(tot_repeats, tiles, false),
                 n_bad = scan(tot_bad, tiles, false);
  CHECK(n_counted + n_repeats + n_bad == n, "%llu + %llu + %llu slots of %llu", (ull)n_counted, (ull)n_repeats, (ull)n_bad, (ull)n);
  const bool full = dm::refuse(entries_before, m->head[dm::kHeadAdded], m->max_keys);
  m->head[dm::kHeadFull] = full;

  // k_vote_commit: nothing when full
  if (!full) {
    std::vector<uint8_t> listed(in.crossed_cap, 0);
    std::vector<uint8_t> was_new(n, 0);  // what every lane loads before its tile's barrier
    for (uint64_t i = 0; i < n; ++i) was_new[i] = leads(i) && lead_id[i] == dm::kNew;
    for (uint32_t i : order) {
      if (!leads(i)) continue;
      const uint64_t tile = i / dm::kTile;
      const uint32_t t = i % dm::kTile;
      uint64_t b_new[dm::kTileWaves] = {}, b_cross[dm::kTileWaves] = {};
      for (uint32_t u = 0; u < dm::kTile; ++u) {
        const uint64_t j = tile * dm::kTile + u;
        if (!leads(j)) continue;
        if (was_new[j]) b_new[u >> 6] |= uint64_t(1) << (u & 63u);
        if (dm::crossed(in.threshold, lead_before[j], after_of(j))) b_cross[u >> 6] |= uint64_t(1) << (u & 63u);
      }
      const bool is_new = (b_new[t >> 6] >> (t & 63u)) & 1u;
      const uint32_t after = after_of(i);
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
  }

  // k_vote_fill: the outputs, and unless full the counted slots' bits
  for (uint32_t i : order) {
    const uint32_t f = first[i];
    out->id[i] = full ? dm::kNoId : lead_id[f];
    if (out->counted) out->counted[i] = counted[i];
    if (out->before) out->before[i] = lead_before[f];
    if (out->after) out->after[i] = lead_before[f] + fresh[f];
    if (counted[i] && !full) {
      const uint32_t v = in.voter[i];
      CHECK(lead_id[f] < m->max_keys && v < m->max_voters, "slot %u marks id %u voter %u", i, lead_id[f], v);
      uint32_t& w = m->mask_at(lead_id[f], v);
      CHECK((w & dv::mask_bit(v)) == 0, "slot %u: voter %u of id %u is counted twice", i, v, lead_id[f]);
      w |= dv::mask_bit(v);
    }
  }
  dv::result_words(n, entries_before, m->head[dm::kHeadAdded], full, m->head[dm::kHeadCrossed], in.crossed_cap, best, n_counted,
                   n_repeats, n_bad, out->r);
  m->head[dm::kHeadEntries] = out->r[1];
  if (full) CHECK(m->bytes() == untouched, "a refused call changed the map");
  m->check();

  for (uint32_t* p : {table, pos, first, lead_id, lead_pos, lead_before, pair_table, pair_pos, counted, fresh, tot_new, tot_cross,
                      tot_counted, tot_repeats, tot_bad})
    std::free(p);
}

// k_vote_lookup
static void run_find_votes(Map& m, const Inputs& in, Outputs* out) {
  const std::vector<uint8_t> untouched = m.bytes();
  for (uint64_t i = 0; i < in.n; ++i) {
    const dm::Found f = walk(m, key_of(in, i));
    const bool found = f.id != dm::kNew;
    const uint32_t v = in.voter[i];
    out->id[i] = found ? f.id : dm::kNoId;
    if (out->before) out->before[i] = found ? m.count[f.id] : 0u;
    out->voted[i] = found && dv::in_range(v, m.max_voters) && (m.mask_at(f.id, v) & dv::mask_bit(v)) != 0;
  }
  CHECK(m.bytes() == untouched, "a find_votes changed the map");
}

static bool same_u32(const uint32_t* a, const uint32_t* b, uint64_t count) {
  return (!a && !b) || count == 0 || (a && b && std::memcmp(a, b, 4 * count) == 0);
}

// what msha_dmap_read and msha_dmap_read_voters return for all entries
static bool same_state(const Map& a, const Map& b) {
  const uint64_t e = a.head[dm::kHeadEntries];
  return e == b.head[dm::kHeadEntries] &&
         (e == 0 || (std::memcmp(a.scope, b.scope, 4 * e) == 0 && std::memcmp(a.digests, b.digests, 32 * e) == 0 &&
                     std::memcmp(a.count, b.count, 4 * e) == 0 && std::memcmp(a.masks, b.masks, 4 * e * a.words) == 0));
}

static void check_units() {
  CHECK(dv::kLaunches == 10 && dv::kResultWords == 11 && dv::kMaxVoters == 1024, "the constants the header text states");
  CHECK(dv::words(1) == 1 && dv::words(31) == 1 && dv::words(32) == 1 && dv::words(33) == 2 && dv::words(64) == 2 &&
            dv::words(65) == 3 && dv::words(1024) == 32,
        "words");
  CHECK(dv::mask_word(0) == 0 && dv::mask_word(31) == 0 && dv::mask_word(32) == 1 && dv::mask_word(1023) == 31, "mask_word");
  CHECK(dv::mask_bit(0) == 1u && dv::mask_bit(31) == 0x80000000u && dv::mask_bit(32) == 1u && dv::mask_bit(63) == 0x80000000u,
        "mask_bit");
  CHECK(dv::in_range(0, 1) && !dv::in_range(1, 1) && dv::in_range(1023, 1024) && !dv::in_range(1024, 1024) &&
            !dv::in_range(0xFFFFFFFFu, 1024),
        "in_range");
  CHECK(dv::counted(true, 0, 5) && !dv::counted(false, 0, 5) && !dv::counted(true, 1u << 5, 5) && dv::counted(true, 1u << 5, 38) &&
            !dv::counted(true, 1u << 5, 37) && dv::counted(true, ~(1u << 31), 63),
        "counted");
  CHECK(dv::pair_same(3, 4, 3, 4) && !dv::pair_same(3, 4, 4, 3) && !dv::pair_same(3, 4, 3, 5) && !dv::pair_same(0, 1u << 31, 0, 0),
        "pair_same");
  CHECK(dv::pair_hash(1, 2, 3) != dv::pair_hash(1, 3, 2) && dv::pair_hash(1, 2, 3) != dv::pair_hash(2, 2, 3), "pair_hash");
  uint64_t r[dv::kResultWords];
  dv::result_words(9, 4, 2, false, 5, 3, gp::best_key(6, 1), 4, 3, 2, r);
  const uint64_t ok[dv::kResultWords] = {9, 6, 2, 0, 5, 3, 6, 1, 4, 3, 2};
  CHECK(std::memcmp(r, ok, sizeof r) == 0, "result_words");
  dv::result_words(9, 4, 2, true, 5, 3, 0, 4, 3, 2, r);
  const uint64_t refused[dv::kResultWords] = {9, 4, 2, 1, 0, 0, 0, 0, 4, 3, 2};
  CHECK(std::memcmp(r, refused, sizeof r) == 0, "result_words of a refused call");
  dv::result_words(2, 0, 1, false, 0, 0, gp::best_key(0, 0), 0, 0, 2, r);  // a key all of whose voters were out of range
  CHECK(r[1] == 1 && r[6] == 0 && r[7] == 0 && r[10] == 2, "result_words of a key without a voter");

  // the store: a plain map's, then the masks; the workspace: an add's, then the vote's
  // arrays in order, each 256-aligned and large enough, none overlapping the next
  std::vector<uint64_t> ks = {1, 2, 3, 4, 8, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300, 4097, 65537};
  for (uint32_t b = 17; b <= 30; ++b) {
    ks.push_back((uint64_t(1) << b) - 1);
    ks.push_back(uint64_t(1) << b);
  }
  for (uint64_t k : ks) {
    for (uint32_t mv : {1u, 31u, 32u, 33u, 64u, 65u, 1024u}) {
      const dv::VoteStore s(k, mv);
      const dm::Store p(k);
      CHECK(s.cap == p.cap && s.head == p.head && s.table == p.table && s.scope == p.scope && s.digests == p.digests &&
                s.count == p.count && s.mask == p.bytes,
            "max_keys %llu: the plain map's arrays stay where they are", (ull)k);
      CHECK(s.mask % 256 == 0 && s.mask_words == dv::words(mv) && s.mask + 4 * s.mask_words * k <= s.bytes && s.bytes % 256 == 0 &&
                (s.bytes - s.mask) % 16 == 0,
            "max_keys %llu max_voters %u: the masks", (ull)k, mv);
    }
    const dv::VoteLayout c(k);  // k as a slot count
    const uint64_t at[9] = {c.pair_table, c.pair_pos, c.counted, c.fresh, c.tot_counted, c.tot_repeats, c.tot_bad, c.head, c.bytes};
    const uint64_t need[8] = {4 * c.pair_cap, 4 * k, 4 * k, 4 * k, 4 * gp::tiles(k), 4 * gp::tiles(k), 4 * gp::tiles(k),
                              8 * dv::kHeadWords};
    CHECK(c.pair_table == c.c.bytes && c.pair_cap == gp::capacity(k), "n %llu: the vote's arrays start behind the add's", (ull)k);
    for (uint32_t j = 0; j < 8; ++j) CHECK(at[j] % 256 == 0 && at[j] + need[j] <= at[j + 1], "n %llu: vote array %u", (ull)k, j);
    // what k_vote_find relies on: its grid reaches every quad of the pair table and of fresh
    CHECK(c.pair_cap / 4 <= gp::tiles(k) * dm::kTile && 16 * ((k + 3) / 4) <= msha::round256(4 * k), "n %llu: find's clearing", (ull)k);
  }
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::printf("usage: dmap_vote_check SEQUENCES RESULTS\n");
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
    int64_t sh[5];
    if (std::fread(sh, 8, 5, in_f) != 5) return 2;
    // three maps, three seeds: where a key and a pair lie differs between them as well
    const uint64_t seeds[3] = {0x1111111111111111ull, 0xFEDCBA9876543210ull, 0x0F0F0F0F0F0F0F0Full + (uint64_t)q};
    Map m0((uint64_t)sh[0], (uint32_t)sh[1], seeds[0], sh[2]), m1((uint64_t)sh[0], (uint32_t)sh[1], seeds[1], sh[2]),
        m2((uint64_t)sh[0], (uint32_t)sh[1], seeds[2], sh[2]);
    for (int64_t s = 0; s < sh[4]; ++s, ++steps_run) {
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
      in.pair_home = sh[3];
      uint8_t* digests = nullptr;
      uint32_t *scope = nullptr, *voter = nullptr;
      if (kind != kClear) {
        std::vector<uint32_t> val(n), flips(2 * n_flips);
        if (!read_words(in_f, val.data(), 4 * n)) return 2;
        if (h[2]) {
          scope = exact<uint32_t>(n);
          if (!read_words(in_f, scope, 4 * n)) return 2;
        }
        voter = exact<uint32_t>(n);
        if (!read_words(in_f, voter, 4 * n)) return 2;
        if (!read_words(in_f, flips.data(), 8 * n_flips)) return 2;
        digests = exact<uint8_t>(32 * n);
        for (uint64_t i = 0; i < n; ++i) base_row(val[i], digests + 32 * i);
        for (uint64_t j = 0; j < n_flips; ++j) digests[32ull * flips[2 * j] + flips[2 * j + 1]] ^= kFlip;
      }
      in.digests = digests;
      in.scope = scope;
      in.voter = voter;

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

      const bool find = kind == kFindVotes;
      Outputs a(in, find), b(in, find), c(in, find);
      if (kind == kVote) {
        run_vote(&m0, in, up, seeds[0] ^ 0x55, &a);
        run_vote(&m1, in, down, seeds[1] ^ 0x55, &b);
        run_vote(&m2, in, mixed, seeds[2] ^ 0x55, &c);
      } else if (find) {
        run_find_votes(m0, in, &a);
        run_find_votes(m1, in, &b);
        run_find_votes(m2, in, &c);
      } else if (kind == kClear) {
        m0.clear();
        m1.clear();
        m2.clear();
        m0.check();
      } else {
        std::printf("unknown step kind %d\n", kind);
        return 2;
      }
      for (const Outputs* o : {&b, &c}) {
        CHECK(same_u32(a.id, o->id, n) && same_u32(a.counted, o->counted, n) && same_u32(a.before, o->before, n) &&
                  same_u32(a.after, o->after, n) && same_u32(a.voted, o->voted, n) &&
                  same_u32(a.crossed, o->crossed, in.crossed_cap) && (kind != kVote || std::memcmp(a.r, o->r, sizeof a.r) == 0),
              "another lane order or seed gives another answer");
      }
      CHECK(same_state(m0, m1) && same_state(m0, m2), "another lane order or seed leaves another map");

      const std::vector<uint32_t> unset(n, kSentinel);
      if (kind == kVote) {
        std::fwrite(a.r, 8, dv::kResultWords, out_f);
        write_u32(out_f, a.id, n);
        write_u32(out_f, a.counted ? a.counted : unset.data(), n);
        write_u32(out_f, a.before ? a.before : unset.data(), n);
        write_u32(out_f, a.after ? a.after : unset.data(), n);
        write_u32(out_f, a.crossed, in.crossed_cap);
      } else if (find) {
        write_u32(out_f, a.id, n);
        write_u32(out_f, a.before ? a.before : unset.data(), n);
        write_u32(out_f, a.voted, n);
      }
      const uint64_t entries = m0.head[dm::kHeadEntries];
      std::fwrite(&entries, 8, 1, out_f);
      write_u32(out_f, m0.scope, entries);
      if (entries) std::fwrite(m0.digests, 32, entries, out_f);
      write_u32(out_f, m0.count, entries);
      write_u32(out_f, m0.masks, entries * m0.words);
      std::free(scope);
      std::free(voter);
      std::free(digests);
    }
  }
  std::fclose(in_f);
  std::fclose(out_f);
  if (g_failed) {
    std::printf("dmap_vote FAILED: %d checks\n", g_failed);
    return 1;
  }
  std::printf("dmap_vote ok: %lld sequences, %llu steps\n", (long long)count, (ull)steps_run);
  return 0;
}
