// Stand-alone check of mirbft_amd/csrc/stream_jobs.hpp (tests/test_dstream_jobs_cpu.py
// builds it with -fsanitize=address,undefined and runs it). The header is everything
// the kernels of stream_jobs.hip run but the wave intrinsics; here a loop over 64 lanes
// stands in for a ballot and plain arrays for LDS.
//
//   stream_jobs_check --tile          prints kTileJobs
//   stream_jobs_check FILE...         each file (tests/dstream_jobs_matrix.py write_ids)
//                                     holds cases of n streams and k job ids
//
// For every case the radix passes are run as the GPU runs them -- per tile a digit
// histogram, an exclusive scan of every digit's row of counts and of the digits' totals,
// per tile the scatter with ranks from ballots and per-wave counts -- with every array a
// heap block of exactly the size stream_jobs.hpp Layout gives it, so the sanitizer sees
// an index outside one. The permutation must equal std::stable_sort's, every in-tile rank the
// header's serial restatement, the CSR a count of the keys. Then the layout is checked
// for k and n up to 2^32 - 2: sizes only, no overflow, no overlap.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <vector>

#include "../../mirbft_amd/csrc/stream_jobs.hpp"

namespace sj = msha::sjobs;

static int g_failed = 0;
#define CHECK(cond, ...)                                      \
  do {                                                        \
    if (!(cond)) {                                            \
      std::printf("FAIL %s:%d: %s: ", name, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                               \
      std::printf("\n");                                      \
      ++g_failed;                                             \
      return;                                                 \
    }                                                         \
  } while (0)

struct Pair {
  uint32_t key, idx;
};

// One pass over k pairs (first: from the ids), as k_sjobs_hist, k_sjobs_scan and
// k_sjobs_scatter do it. counts holds exactly n_counts entries, out exactly k.
static void run_pass(const char* name, const uint32_t* ids, uint64_t n, const Pair* in, Pair* out, uint32_t* counts,
                     const sj::Layout& lay, uint64_t k, uint32_t pass) {
  const uint64_t n_tiles = lay.n_tiles;
  auto load = [&](uint64_t j) { return pass == 0 ? Pair{sj::clamp_key(ids[j], n), (uint32_t)j} : in[j]; };
  // histogram
  for (uint64_t tile = 0; tile < n_tiles; ++tile) {
    uint32_t hist[sj::kDigits] = {};
    for (uint64_t i = 0; i < sj::kTileJobs; ++i) {
      const uint64_t j = tile * sj::kTileJobs + i;
      if (j < k) ++hist[sj::digit(load(j).key, pass)];
    }
    for (uint32_t d = 0; d < sj::kDigits; ++d) counts[sj::count_index(d, tile, n_tiles)] = hist[d];
  }
  // scan: every digit's row for itself, its total behind the rows
  for (uint32_t d = 0; d < sj::kDigits; ++d) {
    uint32_t run = 0;
    for (uint64_t tile = 0; tile < n_tiles; ++tile) {
      uint32_t& c = counts[sj::count_index(d, tile, n_tiles)];
      const uint32_t v = c;
      c = run;
      run += v;
    }
    counts[sj::total_index(d, n_tiles)] = run;
  }
  // what a scatter workgroup does first: the totals' exclusive scan
  uint32_t lower[sj::kDigits], all = 0;
  for (uint32_t d = 0; d < sj::kDigits; ++d) {
    lower[d] = all;
    all += counts[sj::total_index(d, n_tiles)];
  }
  CHECK(all == k, "the counts add up to %u, not %llu", all, (unsigned long long)k);
  // scatter
  for (uint64_t tile = 0; tile < n_tiles; ++tile) {
    static uint32_t wcount[sj::kWaves][sj::kDigits], earlier[sj::kWaves][sj::kDigits];
    static uint32_t rank[sj::kWaves][sj::kRounds][64], digits[sj::kTileJobs];
    std::memset(wcount, 0, sizeof wcount);
    uint32_t in_tile = 0;
    for (uint32_t w = 0; w < sj::kWaves; ++w) {
      for (uint32_t r = 0; r < sj::kRounds; ++r) {
        uint32_t d[64];
        uint64_t valid = 0, bit_ballot[sj::kDigitBits] = {};
        for (uint32_t lane = 0; lane < 64; ++lane) {
          const uint64_t j = tile * sj::kTileJobs + sj::item_index(w, r, lane);
          const bool v = j < k;
          d[lane] = sj::digit(v ? load(j).key : 0, pass);
          if (v) {
            valid |= 1ull << lane;
            CHECK(sj::item_index(w, r, lane) == in_tile, "a tile's jobs are taken in order");
            digits[in_tile++] = d[lane];
          }
          for (uint32_t b = 0; b < sj::kDigitBits; ++b)
            if ((d[lane] >> b) & 1u) bit_ballot[b] |= 1ull << lane;
        }
        uint32_t before[64];
        uint64_t peer_mask[64];
        for (uint32_t lane = 0; lane < 64; ++lane) {  // every lane reads before a leader adds
          peer_mask[lane] = sj::peers(d[lane], bit_ballot, valid);
          before[lane] = wcount[w][d[lane]];
          rank[w][r][lane] = before[lane] + sj::lane_rank(peer_mask[lane], lane);
        }
        for (uint32_t lane = 0; lane < 64; ++lane)
          if (((valid >> lane) & 1) && sj::leads(peer_mask[lane], lane))
            wcount[w][d[lane]] = before[lane] + sj::popcount64(peer_mask[lane]);
      }
    }
    for (uint32_t d = 0; d < sj::kDigits; ++d) {
      uint32_t sum = 0;
      for (uint32_t w = 0; w < sj::kWaves; ++w) {
        earlier[w][d] = sum;
        sum += wcount[w][d];
      }
    }
    for (uint32_t w = 0; w < sj::kWaves; ++w)
      for (uint32_t r = 0; r < sj::kRounds; ++r)
        for (uint32_t lane = 0; lane < 64; ++lane) {
          const uint32_t i = sj::item_index(w, r, lane);
          const uint64_t j = tile * sj::kTileJobs + i;
          if (j >= k) continue;
          const Pair p = load(j);
          const uint32_t d = sj::digit(p.key, pass);
          const uint32_t in_tile_rank = earlier[w][d] + rank[w][r][lane];
          // the serial restatement is quadratic: every job of a small tile, a sample of a full one
          if (in_tile <= 300 || i % 37 == 0 || i + 2 >= in_tile)
            CHECK(in_tile_rank == sj::serial_rank(digits, i), "tile %llu job %u: rank %u", (unsigned long long)tile, i,
                  in_tile_rank);
          const uint64_t pos = sj::scatter_pos(lower[d], counts[sj::count_index(d, tile, n_tiles)], earlier[w][d], rank[w][r][lane]);
          CHECK(pos < k, "position %llu of %llu", (unsigned long long)pos, (unsigned long long)k);
          out[pos] = p;
        }
  }
}

static void run_case(const char* name, uint64_t n, const std::vector<uint32_t>& ids_v) {
  const uint64_t k = ids_v.size();
  if (k == 0) return;
  const sj::Layout lay(k, n);
  CHECK(lay.ok, "layout");
  // heap blocks of exactly the layout's sizes
  std::unique_ptr<uint32_t[]> ids(new uint32_t[k]);
  std::copy(ids_v.begin(), ids_v.end(), ids.get());
  std::unique_ptr<Pair[]> buf[2] = {std::unique_ptr<Pair[]>(new Pair[k]), std::unique_ptr<Pair[]>(new Pair[k])};
  std::unique_ptr<uint32_t[]> counts(new uint32_t[lay.n_counts]);
  CHECK(lay.pairs[1] - lay.pairs[0] >= 8 * k && lay.begin - lay.counts >= 4 * lay.n_counts, "buffer sizes");

  const uint32_t passes = sj::pass_count(n);
  CHECK(passes >= 1 && passes <= 4 && (passes == 4 || (n >> (8 * passes)) == 0) &&
            (passes == 1 || (n >> (8 * (passes - 1))) != 0),
        "pass_count(%llu) = %u", (unsigned long long)n, passes);
  const Pair* in = nullptr;
  for (uint32_t pass = 0; pass < passes; ++pass) {
    Pair* out = buf[sj::pass_output(pass)].get();
    const int failed = g_failed;
    run_pass(name, ids.get(), n, in, out, counts.get(), lay, k, pass);
    if (g_failed != failed) return;
    in = out;
  }
  CHECK(in == buf[sj::sorted_buffer(passes)].get(), "sorted_buffer");

  std::vector<uint32_t> want(k);
  std::iota(want.begin(), want.end(), 0u);
  std::stable_sort(want.begin(), want.end(), [&](uint32_t x, uint32_t y) {
    return sj::clamp_key(ids[x], n) < sj::clamp_key(ids[y], n);
  });
  for (uint64_t p = 0; p < k; ++p) {
    CHECK(in[p].idx == want[p], "position %llu: job %u, stable_sort says %u", (unsigned long long)p, in[p].idx, want[p]);
    CHECK(in[p].key == sj::clamp_key(ids[want[p]], n), "position %llu: key", (unsigned long long)p);
  }

  // the CSR against a count: begin[t] = jobs with a key below t
  auto key_at = [&](uint64_t p) { return in[p].key; };
  std::vector<uint32_t> keys(k);
  for (uint64_t p = 0; p < k; ++p) keys[p] = in[p].key;
  auto count_below = [&](uint64_t t) {
    uint64_t c = 0;
    for (uint64_t p = 0; p < k; ++p) c += keys[p] < t;
    return c;
  };
  std::vector<uint64_t> ts = {0, 1, n / 2, n - 1, n};
  for (uint64_t p = 0; p < k; p += (k > 4000 ? 97 : 1)) {
    ts.push_back(keys[p]);
    ts.push_back((uint64_t)keys[p] + 1 <= n ? keys[p] + 1 : n);
    if (keys[p]) ts.push_back(keys[p] - 1);
  }
  for (uint64_t t : ts) {
    if (t > n) continue;
    const uint64_t b = sj::lower_bound(k, t, key_at);
    CHECK(b == count_below(t), "begin[%llu] = %llu", (unsigned long long)t, (unsigned long long)b);
  }
  if (n <= 70000) {  // every entry, by one running count
    std::vector<uint64_t> hist(n + 2, 0);
    for (uint64_t p = 0; p < k; ++p) ++hist[keys[p] + 1];
    uint64_t c = 0;
    for (uint64_t t = 0; t <= n; ++t) {
      c += hist[t];
      CHECK(sj::lower_bound(k, t, key_at) == c, "begin[%llu]", (unsigned long long)t);
    }
  }
  uint64_t valid = 0;
  for (uint64_t j = 0; j < k; ++j) valid += ids[j] < n;
  CHECK(sj::lower_bound(k, n, key_at) == valid, "begin[n] is the count of valid jobs");
  std::printf("case %s: %llu streams, %llu jobs, %u passes, %llu valid\n", name, (unsigned long long)n,
              (unsigned long long)k, passes, (unsigned long long)valid);
}

static void check_layout() {
  const char* name = "layout";
  const uint64_t top = 0xFFFFFFFEull;
  const uint64_t ks[] = {1, 2, sj::kTileJobs - 1, sj::kTileJobs, sj::kTileJobs + 1, 1310720, 1ull << 31, top};
  const uint64_t ns[] = {1, 255, 256, 65536, 1ull << 24, top};
  for (uint64_t k : ks)
    for (uint64_t n : ns) {
      const sj::Layout lay(k, n);
      CHECK(lay.ok, "k %llu n %llu", (unsigned long long)k, (unsigned long long)n);
      CHECK(lay.n_tiles == (k + sj::kTileJobs - 1) / sj::kTileJobs && lay.n_counts == (lay.n_tiles + 1) * sj::kDigits, "tiles");
      const uint64_t at[7] = {lay.pairs[0], lay.pairs[1], lay.off, lay.len, lay.counts, lay.begin, lay.bytes};
      const uint64_t need[6] = {8 * k, 8 * k, 8 * k, 8 * k, 4 * lay.n_counts, 8 * (n + 1)};
      for (int i = 0; i < 6; ++i) {
        CHECK(at[i] % 64 == 0, "alignment of buffer %d", i);
        CHECK(at[i + 1] >= at[i] && at[i + 1] - at[i] >= need[i] && at[i + 1] - at[i] < need[i] + 64, "size of buffer %d", i);
      }
      // about 32.5 bytes a job and 8 (n + 1)
      CHECK(lay.bytes <= 32 * k + 4 * sj::kDigits * (lay.n_tiles + 1) + 8 * (n + 1) + 6 * 64, "total");
    }
  // a tile count that does not fit: flagged, not wrapped
  CHECK(!sj::Layout(UINT64_MAX - 5, 1).ok, "an overflowing size is refused");
  CHECK(sj::pass_count(1) == 1 && sj::pass_count(255) == 1 && sj::pass_count(256) == 2 && sj::pass_count(65535) == 2 &&
            sj::pass_count(65536) == 3 && sj::pass_count((1ull << 24) - 1) == 3 && sj::pass_count(1ull << 24) == 4 &&
            sj::pass_count(top) == 4,
        "pass_count");
  CHECK(sj::clamp_key(7, 8) == 7 && sj::clamp_key(8, 8) == 8 && sj::clamp_key(0xFFFFFFFFu, 8) == 8 &&
            sj::clamp_key(0xFFFFFFFFu, top) == (uint32_t)top,
        "clamp_key");
  CHECK(sj::digit(0x04030201u, 0) == 1 && sj::digit(0x04030201u, 1) == 2 && sj::digit(0x04030201u, 3) == 4, "digit");
  std::printf("layout ok\n");
}

// A case of its own: ids with all four digits in use on a set of 2^32 - 2 streams.
static void check_wide() {
  std::vector<uint32_t> ids;
  uint32_t x = 12345;
  for (int i = 0; i < 5000; ++i) {
    x = x * 1664525u + 1013904223u;
    ids.push_back(i && i % 9 == 0 ? ids[ids.size() / 2] : i % 50 == 0 ? 0xFFFFFFFFu - (i & 1) : x);
  }
  run_case("wide", 0xFFFFFFFEull, ids);
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "--tile")) {
    std::printf("%u\n", sj::kTileJobs);
    return 0;
  }
  for (int f = 1; f < argc; ++f) {
    FILE* fp = std::fopen(argv[f], "rb");
    if (!fp) {
      std::printf("cannot open %s\n", argv[f]);
      return 2;
    }
    uint64_t n_cases = 0;
    if (std::fread(&n_cases, 8, 1, fp) != 1) return 2;
    for (uint64_t c = 0; c < n_cases; ++c) {
      uint64_t hdr[2];
      if (std::fread(hdr, 8, 2, fp) != 2) return 2;
      std::vector<uint32_t> ids(hdr[1]);
      if (hdr[1] && std::fread(ids.data(), 4, hdr[1], fp) != hdr[1]) return 2;
      const char* base = std::strrchr(argv[f], '/') ? std::strrchr(argv[f], '/') + 1 : argv[f];
      char name[96];
      std::snprintf(name, sizeof name, "%s#%llu", base, (unsigned long long)c);
      run_case(name, hdr[0], ids);
    }
    std::fclose(fp);
  }
  check_wide();
  check_layout();
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("stream_jobs ok\n");
  return 0;
}
