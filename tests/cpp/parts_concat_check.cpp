// Stand-alone check of mirbft_amd/csrc/parts_concat.hpp (tests/test_parts_concat_cpu.py
// builds it with -fsanitize=address,undefined and runs it). The header is the placement
// logic of k_concat_copy; here the workgroup's 256 threads run one after the other, a
// heap array stands in for the LDS image and callbacks for the arena loads and the
// 16-byte stores to d_dst.
//
// For every list of a batch the kernel's loop is replayed (steps, windows, own-thread
// and cooperative fills, granule stores, the carry, the last granule) and checked:
//   1. the message equals a memcpy concatenation of the parts, its pad is zero, and no
//      other byte of d_dst (sentinel-filled, with a margin on both sides) changed;
//   2. every store is one whole granule inside [off, off + round16(len)), and no
//      granule is stored twice;
//   3. in every window each new image byte is written exactly once and no other image
//      byte is written at all (so neighbours never overwrite each other, and the carry
//      survives);
//   4. every load is a multiple of 16 whose granule holds at least one byte of a
//      non-empty part of the list being copied (the read contract of include/mirsha.h).
//      The arena the loads read is a heap block that ends with the last such granule.
//
// Batches: the files tests/parts_concat_matrix.py writes (argv[1..], the ones the GPU
// test launches), and seeded random batches made here with overlapping, repeated and
// shared parts of every size class.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../mirbft_amd/csrc/parts_concat.hpp"

namespace mp = msha::parts;
namespace pc = msha::parts_concat;

static int g_failed = 0;
#define CHECK(cond, ...)                                          \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s: ", name, __LINE__, #cond);     \
      std::printf(__VA_ARGS__);                                   \
      std::printf("\n");                                          \
      ++g_failed;                                                 \
      return;                                                     \
    }                                                             \
  } while (0)

struct Batch {
  std::vector<uint8_t> arena;
  std::vector<uint64_t> off, len, begin;  // begin: n_lists + 1
};

static const uint8_t kSentinel = 0xA5;
static const uint64_t kMargin = 64;
typedef unsigned long long ull;

// One list -> one message at `moff` (a multiple of 16) of dst.
static void check_list(const char* name, const Batch& B, uint64_t s, const uint8_t* heap, uint64_t extent,
                       uint64_t* loads_out) {
  const uint64_t j0 = B.begin[s], np = B.begin[s + 1] - j0;
  std::vector<uint8_t> msg;
  std::vector<uint8_t> allowed(extent, 0);
  for (uint64_t j = j0; j < j0 + np; ++j) {
    msg.insert(msg.end(), B.arena.begin() + B.off[j], B.arena.begin() + B.off[j] + B.len[j]);
    if (B.len[j])
      for (uint64_t g = B.off[j] / 16; g <= (B.off[j] + B.len[j] - 1) / 16; ++g) allowed[g] = 1;
  }
  const uint64_t total = msg.size(), padded = pc::round16(total);
  const uint64_t moff = 16 * (s % 5);
  std::vector<uint8_t> dst(kMargin + moff + padded + kMargin, kSentinel);
  std::vector<uint8_t> stored(padded / 16, 0);
  uint8_t* const out = dst.data() + kMargin + moff;

  uint64_t bad_loads = 0, loads = 0;
  auto load = [&](uint64_t off) {
    ++loads;
    mp::Granule g{};
    if (off % 16 || off / 16 >= extent || !allowed[off / 16]) {
      ++bad_loads;  // not performed: the contract is already broken
      return g;
    }
    std::memcpy(g.d, heap + off, 16);  // little-endian host, as the GPU
    return g;
  };
  // the image: heap memory, so the sanitizer sees a write past it
  std::vector<uint8_t> img(pc::kImageBytes, 0xC3);
  std::vector<uint8_t> hits(pc::kImageBytes, 0);
  uint64_t bad_image = 0;
  auto st8 = [&](uint32_t x, uint32_t v) {
    if (x >= pc::kImageBytes || v > 0xffu) {
      ++bad_image;
      return;
    }
    img[x] = (uint8_t)v;
    if (hits[x] < 255) ++hits[x];
  };
  auto st32 = [&](uint32_t d, uint32_t v) {
    if (d >= pc::kImageBytes / 4) {
      ++bad_image;
      return;
    }
    std::memcpy(img.data() + 4 * d, &v, 4);
    for (int b = 0; b < 4; ++b)
      if (hits[4 * d + b] < 255) ++hits[4 * d + b];
  };
  uint64_t bad_stores = 0;
  auto store = [&](uint64_t granule, const uint8_t* v) {
    if (granule >= stored.size() || stored[granule]) {
      ++bad_stores;
      return;
    }
    stored[granule] = 1;
    std::memcpy(out + 16 * granule, v, 16);
  };

  const uint32_t S = pc::kStepParts;
  uint64_t base = 0;
  std::vector<uint64_t> off(S), len(S), pos(S);
  for (uint64_t p0 = 0; p0 < np; p0 += S) {
    uint64_t step = 0;
    for (uint32_t t = 0; t < S; ++t) {  // the block-exclusive scan of the step's lengths
      off[t] = len[t] = 0;
      if (p0 + t < np) {
        off[t] = B.off[j0 + p0 + t];
        len[t] = B.len[j0 + p0 + t];
      }
      pos[t] = base + step;
      step += len[t];
    }
    const uint64_t step_end = base + step;
    uint64_t cur = base;
    while (cur < step_end) {
      const pc::Window w = pc::window_at(cur, step_end);
      CHECK(w.wb % 16 == 0 && w.wb <= w.lo && w.lo < w.hi && w.hi - w.wb <= pc::kImageBytes && w.hi <= step_end,
            "list %llu: window [%llu, %llu) from %llu", (ull)s, (ull)w.lo, (ull)w.hi, (ull)w.wb);
      std::fill(hits.begin(), hits.end(), 0);
      for (uint32_t t = 0; t < S; ++t) {
        if (len[t] >= pc::kLargePart) continue;
        const pc::Piece pp = pc::clip(pos[t], len[t], w);
        if (pp.n) pc::copy_piece(off[t] + pp.skip, pp.n, (uint32_t)(pos[t] + pp.skip - w.wb), load, st32, st8);
      }
      for (uint32_t l = 0; l < S; ++l) {
        if (len[l] < pc::kLargePart) continue;
        const pc::Piece pp = pc::clip(pos[l], len[l], w);
        for (uint32_t t = 0; t < S; ++t)
          pc::coop_piece(off[l] + pp.skip, pp.n, (uint32_t)(pos[l] + pp.skip - w.wb), t, S, load, st32, st8);
      }
      for (uint32_t x = 0; x < pc::kImageBytes; ++x) {
        const bool fresh = x >= w.lo - w.wb && x < w.hi - w.wb;
        CHECK(hits[x] == (fresh ? 1 : 0), "list %llu: window at %llu: image byte %u written %u times", (ull)s,
              (ull)w.wb, x, (unsigned)hits[x]);
      }
      const uint32_t ng = pc::window_granules(w), rest = pc::window_rest(w);
      for (uint32_t g = 0; g < ng; ++g) store((w.wb >> 4) + g, img.data() + 16 * g);
      uint8_t carry[16];
      for (uint32_t t = 0; t < rest; ++t) carry[t] = img[16 * ng + t];
      for (uint32_t t = 0; t < rest; ++t) img[t] = carry[t];
      CHECK(((w.hi - rest) & 15) == 0, "list %llu: the carry does not start on a granule", (ull)s);
      cur = w.hi;
    }
    base = step_end;
  }
  CHECK(base == total, "list %llu: %llu bytes placed, %llu expected", (ull)s, (ull)base, (ull)total);
  const uint32_t r = (uint32_t)(base & 15);
  if (r) {
    uint32_t v[4];
    std::memcpy(v, img.data(), 16);
    pc::last_granule(v, r);
    uint8_t b[16];
    std::memcpy(b, v, 16);
    store(base >> 4, b);
  }
  CHECK(bad_image == 0, "list %llu: %llu writes outside the image", (ull)s, (ull)bad_image);
  CHECK(bad_stores == 0, "list %llu: %llu stores outside the message or repeated", (ull)s, (ull)bad_stores);
  CHECK(bad_loads == 0, "list %llu: %llu of %llu loads outside the granules of its non-empty parts", (ull)s,
        (ull)bad_loads, (ull)loads);
  for (size_t g = 0; g < stored.size(); ++g) CHECK(stored[g], "list %llu: granule %zu never stored", (ull)s, g);
  for (uint64_t i = 0; i < total; ++i)
    CHECK(out[i] == msg[i], "list %llu (%llu bytes): byte %llu is %02x, expected %02x", (ull)s, (ull)total, (ull)i,
          out[i], msg[i]);
  for (uint64_t i = total; i < padded; ++i) CHECK(out[i] == 0, "list %llu: pad byte %llu is %02x", (ull)s, (ull)i, out[i]);
  for (uint64_t i = 0; i < kMargin + moff; ++i) CHECK(dst[i] == kSentinel, "list %llu: a byte before the message written", (ull)s);
  for (uint64_t i = kMargin + moff + padded; i < dst.size(); ++i)
    CHECK(dst[i] == kSentinel, "list %llu: a byte after the pad written", (ull)s);
  *loads_out += loads;
}

static void check_batch(const char* name, const Batch& B) {
  const uint64_t n_parts = B.off.size();
  CHECK(B.len.size() == n_parts && !B.begin.empty() && B.begin.back() <= n_parts, "inputs of the batch");
  uint64_t extent = 0;
  for (uint64_t j = 0; j < n_parts; ++j)
    if (B.len[j]) {
      CHECK(B.off[j] + B.len[j] <= B.arena.size(), "part %llu outside the arena", (ull)j);
      extent = std::max<uint64_t>(extent, (B.off[j] + B.len[j] + 15) / 16);
    }
  // what the loads read: exactly [0, 16 * extent), zero-filled past the arena's end
  uint8_t* heap = static_cast<uint8_t*>(std::malloc(extent ? 16 * extent : 1));
  std::memset(heap, 0, extent ? 16 * extent : 1);
  std::memcpy(heap, B.arena.data(), std::min<uint64_t>(B.arena.size(), 16 * extent));
  const uint64_t n = B.begin.size() - 1;
  uint64_t loads = 0;
  for (uint64_t s = 0; s < n && !g_failed; ++s) {
    if (B.begin[s + 1] < B.begin[s]) {
      std::printf("FAIL %s: list %llu decreases\n", name, (ull)s);
      ++g_failed;
      break;
    }
    check_list(name, B, s, heap, extent, &loads);
  }
  std::free(heap);
  if (!g_failed)
    std::printf("%s: %llu lists, %llu parts, %llu loads ok\n", name, (ull)n, (ull)n_parts, (ull)loads);
}

// tests/parts_matrix.py write_batch(): little-endian u64 arena_len, n_parts, n_lists,
// then the arena, part_off, part_len and the lists' part begin (n_lists + 1).
static bool read_batch(const char* path, Batch* B) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  uint64_t h[3];
  bool ok = std::fread(h, 8, 3, f) == 3 && h[0] < (1ull << 30) && h[1] < (1ull << 26) && h[2] < (1ull << 26);
  if (ok) {
    B->arena.resize(h[0]);
    B->off.resize(h[1]);
    B->len.resize(h[1]);
    B->begin.resize(h[2] + 1);
    ok = std::fread(B->arena.data(), 1, h[0], f) == h[0] && std::fread(B->off.data(), 8, h[1], f) == h[1] &&
         std::fread(B->len.data(), 8, h[1], f) == h[1] && std::fread(B->begin.data(), 8, h[2] + 1, f) == h[2] + 1;
  }
  std::fclose(f);
  return ok;
}

// Random batches: parts anywhere in a small arena (so they overlap), some repeated
// within a list, some shared between lists; empty, tiny, mid-sized, around the
// large-part threshold and a few past the image size; lists of up to three steps.
static Batch random_batch(uint32_t seed) {
  std::mt19937_64 rng(seed);
  Batch B;
  B.arena.resize(40000 + rng() % 64);
  for (auto& b : B.arena) b = (uint8_t)rng();
  const uint64_t n = 12;
  B.begin.push_back(0);
  for (uint64_t a = 0; a < n; ++a) {
    const uint64_t k = a % 4 == 0 ? rng() % (3 * pc::kStepParts) : rng() % 40;
    for (uint64_t p = 0; p < k; ++p) {
      if (!B.off.empty() && rng() % 4 == 0) {  // an earlier part again (this list's or another's)
        const uint64_t j = rng() % B.off.size();
        B.off.push_back(B.off[j]);
        B.len.push_back(B.len[j]);
        continue;
      }
      const uint64_t kind = rng() % 16;
      const uint64_t len = kind == 0   ? 0
                           : kind < 6  ? 1 + rng() % 40
                           : kind < 12 ? rng() % 400
                           : kind < 15 ? pc::kLargePart - 20 + rng() % 40
                                       : rng() % (2 * pc::kImageBytes + 100);
      const uint64_t off = rng() % (B.arena.size() - len + 1);
      B.off.push_back(off);
      B.len.push_back(len);
    }
    B.begin.push_back(B.off.size());
  }
  return B;
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc && !g_failed; ++i) {
    Batch B;
    if (!read_batch(argv[i], &B)) {
      std::printf("FAIL cannot read %s\n", argv[i]);
      return 2;
    }
    check_batch("matrix", B);
  }
  for (uint32_t seed = 1; seed <= 12 && !g_failed; ++seed) check_batch("random", random_batch(seed));
  {  // parts that end exactly at the arena's last byte and start at its first
    Batch B;
    B.arena.resize(131);
    for (size_t i = 0; i < B.arena.size(); ++i) B.arena[i] = (uint8_t)(i * 7 + 1);
    B.off = {0, 130, 0, 67, 131, 3};
    B.len = {131, 1, 1, 64, 0, 128};
    B.begin = {0, 1, 2, 3, 4, 5, 6, 6};
    check_batch("edges", B);
  }
  if (g_failed) return 1;
  std::printf("parts_concat ok\n");
  return 0;
}
