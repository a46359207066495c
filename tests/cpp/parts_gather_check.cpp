// Stand-alone check of mirbft_amd/csrc/parts_gather.hpp (tests/test_parts_gather.py
// builds it with -fsanitize=address,undefined and runs it). The header is what one
// lane of k_digest_parts runs to assemble its action's blocks; here a plain array
// stands in for the lane's LDS slot and a callback for the 16-byte load.
//
// For every action of a batch the block loop of the kernel is replayed on the host
// (fill_block, then the tail and length blocks as sha256_device.hpp builds them) and
// checked against a memcpy concatenation of the parts:
//   1. the sixteen big-endian words of every block, padding blocks included, equal
//      those of the concatenation padded per FIPS 180-4 5.1.1, byte by byte;
//   2. every offset handed to the load callback is a multiple of 16 whose granule
//      holds at least one byte of a non-empty part (the read contract of
//      include/mirsha.h, checked exactly). The arena the loads read is a heap block
//      that begins at offset 0 and ends with the last such granule, so the sanitizer
//      sees a read before or after it as well.
//
// Batches: the boundary matrix tests/parts_matrix.py writes (argv[1], the one the GPU
// test launches), and seeded random batches made here with overlapping, repeated and
// shared parts.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../mirbft_amd/csrc/parts_gather.hpp"

namespace mp = msha::parts;

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
  std::vector<uint64_t> off, len, begin;  // begin: n_actions + 1
};

static uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }

// sha256_device.hpp build_tail / length_block / to_words, restated for the host.
static int build_tail_host(const uint32_t (&raw)[16], uint32_t r, uint64_t len, uint32_t (&w)[16]) {
  for (int j = 0; j < 16; ++j) {
    const int k = (int)r - 4 * j;
    const uint32_t keep = k >= 4 ? 0xffffffffu : (k <= 0 ? 0u : (0xffffffffu >> (32 - 8 * k)));
    const uint32_t pad = (k >= 0 && k < 4) ? (0x80u << (8 * k)) : 0u;
    w[j] = bswap32((raw[j] & keep) | pad);
  }
  const uint64_t bits = len * 8;
  if (r < 56) {
    w[14] = (uint32_t)(bits >> 32);
    w[15] = (uint32_t)bits;
    return 0;
  }
  return 1;
}

// The blocks of a message padded per FIPS 180-4 5.1.1, as big-endian words.
static std::vector<uint32_t> padded_words(const std::vector<uint8_t>& msg) {
  std::vector<uint8_t> p = msg;
  p.push_back(0x80);
  while (p.size() % 64 != 56) p.push_back(0);
  const uint64_t bits = (uint64_t)msg.size() * 8;
  for (int i = 7; i >= 0; --i) p.push_back((uint8_t)(bits >> (8 * i)));
  std::vector<uint32_t> w(p.size() / 4);
  for (size_t i = 0; i < w.size(); ++i)
    w[i] = ((uint32_t)p[4 * i] << 24) | ((uint32_t)p[4 * i + 1] << 16) | ((uint32_t)p[4 * i + 2] << 8) | p[4 * i + 3];
  return w;
}

static void check_batch(const char* name, const Batch& B) {
  const uint64_t n_parts = B.off.size();
  CHECK(B.len.size() == n_parts && !B.begin.empty() && B.begin.back() <= n_parts, "inputs of the batch");
  // granules that hold a byte of a non-empty part: the only ones a load may name
  uint64_t extent = 0;
  for (uint64_t j = 0; j < n_parts; ++j)
    if (B.len[j]) {
      CHECK(B.off[j] + B.len[j] <= B.arena.size(), "part %llu outside the arena", (unsigned long long)j);
      extent = std::max<uint64_t>(extent, (B.off[j] + B.len[j] + 15) / 16);
    }
  std::vector<uint8_t> allowed(extent, 0);
  for (uint64_t j = 0; j < n_parts; ++j)
    if (B.len[j])
      for (uint64_t g = B.off[j] / 16; g <= (B.off[j] + B.len[j] - 1) / 16; ++g) allowed[g] = 1;
  // what the loads read: exactly [0, 16 * extent), zero-filled past the arena's end
  // (those bytes belong to no part; a device arena has its slack there)
  uint8_t* heap = static_cast<uint8_t*>(std::malloc(extent ? 16 * extent : 1));
  std::memset(heap, 0, extent ? 16 * extent : 1);
  std::memcpy(heap, B.arena.data(), std::min<uint64_t>(B.arena.size(), 16 * extent));

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

  const uint64_t n = B.begin.size() - 1;
  for (uint64_t a = 0; a < n && !g_failed; ++a) {
    std::vector<uint8_t> msg;
    for (uint64_t j = B.begin[a]; j < B.begin[a + 1]; ++j)
      msg.insert(msg.end(), B.arena.begin() + B.off[j], B.arena.begin() + B.off[j] + B.len[j]);
    const std::vector<uint32_t> want = padded_words(msg);

    // the kernel's block loop
    uint32_t slot[16];
    for (auto& x : slot) x = 0xA5C3F00Du;  // an LDS slot starts with whatever was there
    auto slot_write = [&](uint32_t j, uint32_t v) {
      if (j >= 16) {
        std::printf("FAIL %s: action %llu wrote slot dword %u\n", name, (unsigned long long)a, j);
        ++g_failed;
        return;
      }
      slot[j] = v;
    };
    mp::Cursor c;
    mp::cursor_init(c, B.begin[a], (uint32_t)(B.begin[a + 1] - B.begin[a]), B.off.data(), B.len.data());
    std::vector<uint32_t> got;
    uint64_t total = 0;
    int phase = 0;
    while (phase != 2) {
      uint32_t w[16];
      if (phase == 0) {
        const uint32_t r = mp::fill_block(c, B.off.data(), B.len.data(), slot_write, load);
        CHECK(r <= 64, "action %llu: fill_block returned %u", (unsigned long long)a, r);
        total += r;
        if (r == 64) {
          for (int j = 0; j < 16; ++j) w[j] = bswap32(slot[j]);
        } else {
          phase = build_tail_host(slot, r, total, w) ? 1 : 2;
        }
      } else {
        for (int j = 0; j < 14; ++j) w[j] = 0;
        w[14] = (uint32_t)((total * 8) >> 32);
        w[15] = (uint32_t)(total * 8);
        phase = 2;
      }
      got.insert(got.end(), w, w + 16);
      CHECK(got.size() <= want.size(), "action %llu: more blocks than the padded message has", (unsigned long long)a);
    }
    CHECK(total == msg.size(), "action %llu: %llu bytes gathered, %zu expected", (unsigned long long)a,
          (unsigned long long)total, msg.size());
    CHECK(got.size() == want.size(), "action %llu: %zu words, %zu expected", (unsigned long long)a, got.size(),
          want.size());
    for (size_t i = 0; i < got.size(); ++i)
      CHECK(got[i] == want[i], "action %llu (%zu bytes): word %zu is %08x, expected %08x", (unsigned long long)a,
            msg.size(), i, got[i], want[i]);
    CHECK(c.rem == 0 && c.left == 0 && c.j == B.begin[a + 1], "action %llu: cursor not at the end", (unsigned long long)a);
  }
  std::free(heap);
  CHECK(bad_loads == 0, "%llu of %llu loads outside the granules of non-empty parts", (unsigned long long)bad_loads,
        (unsigned long long)loads);
  std::printf("%s: %llu actions, %llu parts, %llu loads ok\n", name, (unsigned long long)n, (unsigned long long)n_parts,
              (unsigned long long)loads);
}

// tests/parts_matrix.py write_batch(): little-endian u64 arena_len, n_parts, n_actions,
// then the arena, part_off, part_len and action_part_begin (n_actions + 1).
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
// within an action, some shared between actions, many empty or tiny.
static Batch random_batch(uint32_t seed) {
  std::mt19937_64 rng(seed);
  Batch B;
  B.arena.resize(700 + rng() % 64);
  for (auto& b : B.arena) b = (uint8_t)rng();
  const uint64_t n = 120;
  B.begin.push_back(0);
  for (uint64_t a = 0; a < n; ++a) {
    const uint64_t k = rng() % 9;
    for (uint64_t p = 0; p < k; ++p) {
      if (!B.off.empty() && rng() % 4 == 0) {  // an earlier part again (this action's or another's)
        const uint64_t j = rng() % B.off.size();
        B.off.push_back(B.off[j]);
        B.len.push_back(B.len[j]);
        continue;
      }
      const uint64_t kind = rng() % 4;
      const uint64_t len = kind == 0 ? 0 : kind == 1 ? 1 + rng() % 4 : kind == 2 ? rng() % 70 : rng() % 300;
      const uint64_t off = rng() % (B.arena.size() - len + 1);
      B.off.push_back(off);
      B.len.push_back(len);
    }
    B.begin.push_back(B.off.size());
  }
  return B;
}

int main(int argc, char** argv) {
  if (argc > 1) {
    Batch B;
    if (!read_batch(argv[1], &B)) {
      std::printf("FAIL cannot read %s\n", argv[1]);
      return 2;
    }
    check_batch("matrix", B);
  }
  for (uint32_t seed = 1; seed <= 40 && !g_failed; ++seed) check_batch("random", random_batch(seed));
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
  std::printf("parts_gather ok\n");
  return 0;
}
