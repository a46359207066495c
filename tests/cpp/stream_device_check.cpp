// Stand-alone check of mirbft_amd/csrc/stream_device.hpp (tests/test_dstream_cpu.py
// builds it with -fsanitize=address,undefined and runs it). The header is what one lane
// of k_dstream_write runs; here a plain array stands in for the lane's LDS slot, a
// callback for the 16-byte loads and a host SHA-256 for compress().
//
// A file (tests/dstream_matrix.py write_rounds) holds the rounds of writes to one set of
// streams. For every row of every round the kernel's write is replayed -- write_row,
// then the tail, state and length update -- and compared with a restatement that
// memcpy-concatenates the stream's buffered bytes and the row's parts and hashes the
// whole blocks: state words, the 64 tail bytes (zero past length % 64) and the length
// must be equal. After each round every stream's sum, computed as k_dstream_finish
// does, must equal the digest in the file (hashlib's).
//
// What the loads may read is enforced twice: every arena offset handed to the load
// callback must be a multiple of 16 whose granule holds a byte of a non-empty part,
// and the arena the loads read is a heap block of exactly the contract's size (the
// last part's end plus MSHA_DEVICE_ARENA_SLACK), each stream's tail row a heap block of
// its own 64 bytes, so the sanitizer sees a read outside either.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../mirbft_amd/csrc/stream_device.hpp"

namespace mp = msha::parts;
namespace ds = msha::dstream;

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

constexpr uint64_t kSlack = 64;  // MSHA_DEVICE_ARENA_SLACK

// ---- SHA-256 for the host (FIPS 180-4 6.2.2) --------------------------------
static const uint32_t K[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
static const uint32_t kIV[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                                0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};

static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
static uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }

// One block of 16 big-endian words into the state.
static void compress(uint32_t (&h)[8], const uint32_t (&w16)[16]) {
  uint32_t w[64];
  for (int i = 0; i < 16; ++i) w[i] = w16[i];
  for (int i = 16; i < 64; ++i) {
    const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
    const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
    w[i] = w[i - 16] + s0 + w[i - 7] + s1;
  }
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
  for (int i = 0; i < 64; ++i) {
    const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
    const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
    hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

// A block of 64 bytes in memory order.
static void compress_bytes(uint32_t (&h)[8], const uint8_t* p) {
  uint32_t w[16];
  for (int i = 0; i < 16; ++i)
    w[i] = ((uint32_t)p[4 * i] << 24) | ((uint32_t)p[4 * i + 1] << 16) | ((uint32_t)p[4 * i + 2] << 8) | p[4 * i + 3];
  compress(h, w);
}

// sha256_device.hpp build_tail, restated for the host.
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

// ---- a set of streams as the kernels keep it ---------------------------------
struct Stream {
  uint32_t state[8];
  std::unique_ptr<uint8_t[]> tail;  // 64 bytes of its own on the heap
  uint64_t length = 0;
  Stream() : tail(new uint8_t[64]) {
    std::memcpy(state, kIV, sizeof state);
    std::memset(tail.get(), 0, 64);
  }
};

struct Round {
  std::vector<uint8_t> arena;
  std::vector<uint64_t> off, len, begin;
  std::vector<uint32_t> rows;
  bool has_rows = false;
  std::vector<uint8_t> digests;   // 32 x n_streams, after the round
  std::vector<uint64_t> lengths;  // n_streams
};

// k_dstream_finish's sum.
static void sum_stream(const Stream& s, uint8_t* out) {
  uint32_t h[8], raw[16], w[16];
  std::memcpy(h, s.state, sizeof h);
  std::memcpy(raw, s.tail.get(), 64);  // little-endian host, as the GPU
  const uint32_t t = (uint32_t)s.length & 63u;
  if (build_tail_host(raw, t, s.length, w)) {
    compress(h, w);
    for (int j = 0; j < 14; ++j) w[j] = 0;
    w[14] = (uint32_t)((s.length * 8) >> 32);
    w[15] = (uint32_t)(s.length * 8);
  }
  compress(h, w);
  for (int j = 0; j < 8; ++j) {
    const uint32_t v = bswap32(h[j]);
    std::memcpy(out + 4 * j, &v, 4);
  }
}

static void check_round(const char* name, std::vector<Stream>& set, const Round& R, uint64_t* loads_out) {
  const uint64_t n_parts = R.off.size(), n_rows = R.begin.size() - 1;
  uint64_t end = 0;
  for (uint64_t j = 0; j < n_parts; ++j)
    if (R.len[j]) {
      CHECK(R.off[j] + R.len[j] + kSlack <= R.arena.size(), "part %llu and its slack outside the arena", (unsigned long long)j);
      end = std::max<uint64_t>(end, R.off[j] + R.len[j]);
    }
  // the contract's arena: everything up to the last part's end and the slack after it
  const uint64_t heap_len = end ? end + kSlack : 1;
  std::unique_ptr<uint8_t[]> heap(new uint8_t[heap_len]);
  std::memcpy(heap.get(), R.arena.data(), std::min<uint64_t>(heap_len, R.arena.size()));
  std::vector<uint8_t> allowed((end + 15) / 16, 0);
  for (uint64_t j = 0; j < n_parts; ++j)
    if (R.len[j])
      for (uint64_t g = R.off[j] / 16; g <= (R.off[j] + R.len[j] - 1) / 16; ++g) allowed[g] = 1;

  uint64_t loads = 0, bad_loads = 0, tail_loads = 0;
  for (uint64_t r = 0; r < n_rows && !g_failed; ++r) {
    const uint64_t s = R.has_rows ? R.rows[r] : r;
    if (s >= set.size()) continue;  // the kernel flags it and touches nothing
    const uint64_t j0 = R.begin[r], jend = R.begin[r + 1];
    if (!ds::range_ok(j0, jend)) continue;
    CHECK(jend <= n_parts, "row %llu names parts past the list", (unsigned long long)r);
    Stream& S = set[s];
    const uint32_t t = (uint32_t)S.length & 63u;

    // the restatement: buffered bytes and parts concatenated, whole blocks hashed
    std::vector<uint8_t> msg(S.tail.get(), S.tail.get() + t);
    for (uint64_t j = j0; j < jend; ++j)
      msg.insert(msg.end(), R.arena.begin() + R.off[j], R.arena.begin() + R.off[j] + R.len[j]);
    uint32_t want_state[8];
    std::memcpy(want_state, S.state, sizeof want_state);
    const uint64_t whole = msg.size() / 64;
    for (uint64_t b = 0; b < whole; ++b) compress_bytes(want_state, msg.data() + 64 * b);
    uint8_t want_tail[64] = {0};
    if (msg.size() % 64) std::memcpy(want_tail, msg.data() + 64 * whole, msg.size() % 64);
    const uint64_t want_len = S.length + (msg.size() - t);

    // the kernel's row
    uint32_t slot[16];
    for (auto& x : slot) x = 0xA5C3F00Du;  // an LDS slot starts with whatever was there
    auto slot_write = [&](uint32_t j, uint32_t v) {
      if (j >= 16) {
        std::printf("FAIL %s: row %llu wrote slot dword %u\n", name, (unsigned long long)r, j);
        ++g_failed;
        return;
      }
      slot[j] = v;
    };
    bool stored = false;  // no tail load may follow a store to the row
    bool late_tail_load = false;
    auto load = [&](uint64_t off) {
      mp::Granule g{};
      if (ds::tagged(off)) {
        ++tail_loads;
        if (stored) late_tail_load = true;
      } else {
        ++loads;
        if (off % 16 || off / 16 >= allowed.size() || !allowed[off / 16]) {
          ++bad_loads;  // not performed: the contract is already broken
          return g;
        }
      }
      std::memcpy(g.d, ds::tagged_address(off, heap.get(), S.tail.get()), 16);  // little-endian host, as the GPU
      return g;
    };
    uint32_t st[8];
    std::memcpy(st, S.state, sizeof st);
    auto block = [&]() {
      stored = true;  // from here on the kernel could as well have overwritten the row
      uint32_t w[16];
      for (int j = 0; j < 16; ++j) w[j] = bswap32(slot[j]);
      compress(st, w);
    };
    const ds::Written wr = ds::write_row(t, j0, (uint32_t)(jend - j0), R.off.data(), R.len.data(), slot_write, load, block);
    CHECK(!late_tail_load, "row %llu read its tail row after the first block", (unsigned long long)r);
    CHECK(wr.tail < 64, "row %llu: a tail of %u bytes", (unsigned long long)r, wr.tail);
    if (wr.appended != 0) {
      uint32_t d[16];
      for (uint32_t j = 0; j < 16; ++j) d[j] = ds::tail_dword(slot[j], j, wr.tail);
      std::memcpy(S.tail.get(), d, 64);
      if (wr.blocks) std::memcpy(S.state, st, sizeof st);
      S.length += wr.appended;
    }
    CHECK(S.length == want_len, "row %llu: length %llu, expected %llu", (unsigned long long)r,
          (unsigned long long)S.length, (unsigned long long)want_len);
    CHECK(wr.blocks == whole, "row %llu: %u blocks, expected %llu", (unsigned long long)r, wr.blocks,
          (unsigned long long)whole);
    CHECK(std::memcmp(S.state, want_state, 32) == 0, "row %llu: state differs", (unsigned long long)r);
    CHECK(std::memcmp(S.tail.get(), want_tail, 64) == 0, "row %llu (t %u, %llu appended): tail row differs",
          (unsigned long long)r, t, (unsigned long long)wr.appended);
  }
  if (g_failed) return;
  CHECK(bad_loads == 0, "%llu of %llu loads outside the granules of non-empty parts", (unsigned long long)bad_loads,
        (unsigned long long)loads);
  for (uint64_t s = 0; s < set.size(); ++s) {
    uint8_t got[32];
    sum_stream(set[s], got);
    CHECK(set[s].length == R.lengths[s], "stream %llu: length %llu, the file has %llu", (unsigned long long)s,
          (unsigned long long)set[s].length, (unsigned long long)R.lengths[s]);
    CHECK(std::memcmp(got, &R.digests[32 * s], 32) == 0, "stream %llu (length %llu): digest differs from the file's",
          (unsigned long long)s, (unsigned long long)set[s].length);
  }
  *loads_out += loads + tail_loads;
}

static bool read_exact(std::FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }

static void check_file(const char* path) {
  const char* name = path;
  std::FILE* f = std::fopen(path, "rb");
  CHECK(f != nullptr, "cannot open");
  uint64_t h[2];
  bool ok = read_exact(f, h, 16) && h[0] >= 1 && h[0] < (1ull << 24) && h[1] < 64;
  std::vector<Stream> set(ok ? h[0] : 0);
  uint64_t loads = 0, rows = 0;
  for (uint64_t k = 0; ok && k < h[1] && !g_failed; ++k) {
    Round R;
    uint64_t q[4];
    ok = read_exact(f, q, 32) && q[0] < (1ull << 30) && q[1] < (1ull << 26) && q[2] < (1ull << 26) && q[3] <= 1;
    if (!ok) break;
    R.arena.resize(q[0]);
    R.off.resize(q[1]);
    R.len.resize(q[1]);
    R.begin.resize(q[2] + 1);
    R.has_rows = q[3] == 1;
    R.rows.resize(R.has_rows ? q[2] : 0);
    R.digests.resize(32 * h[0]);
    R.lengths.resize(h[0]);
    ok = read_exact(f, R.arena.data(), q[0]) && read_exact(f, R.off.data(), 8 * q[1]) &&
         read_exact(f, R.len.data(), 8 * q[1]) && read_exact(f, R.begin.data(), 8 * (q[2] + 1)) &&
         read_exact(f, R.rows.data(), 4 * R.rows.size()) && read_exact(f, R.digests.data(), R.digests.size()) &&
         read_exact(f, R.lengths.data(), 8 * h[0]) && (R.has_rows || q[2] == h[0]);
    if (!ok) break;
    check_round(name, set, R, &loads);
    rows += q[2];
  }
  std::fclose(f);
  CHECK(ok, "not a rounds file");
  if (!g_failed)
    std::printf("rounds: %llu streams, %llu rounds, %llu rows, %llu loads ok\n", (unsigned long long)h[0],
                (unsigned long long)h[1], (unsigned long long)rows, (unsigned long long)loads);
}

// What no file holds: a length past 2^32, and a part offset that carries the tag.
static void check_edges() {
  const char* name = "edges";
  CHECK(ds::kTailTag % 16 == 0 && ds::tagged(ds::kTailTag + 48) && !ds::tagged(ds::kTailTag - 1), "the tag");
  const uint64_t tagged_offs[] = {ds::kTailTag, ds::kTailTag + 16, ds::kTailTag + 48, ~uint64_t(15),
                                  ds::kTailTag + (uint64_t(1) << 40)};
  uint8_t row[64], arena[16];
  for (uint64_t off : tagged_offs) {
    CHECK(ds::tail_granule(off) <= 48 && ds::tail_granule(off) % 16 == 0, "a tagged load leaves the row");
    CHECK(ds::tagged_address(off, arena, row) == row + ds::tail_granule(off), "a tagged offset reads the row");
  }
  CHECK(ds::tagged_address(0, arena, row) == arena, "an untagged offset reads the arena");
  CHECK(ds::range_ok(5, 5) && ds::range_ok(0, 0xffffffffull) && !ds::range_ok(0, 0x100000000ull) && !ds::range_ok(6, 5),
        "range_ok");
  CHECK(ds::tail_dword(0xAABBCCDDu, 0, 4) == 0xAABBCCDDu && ds::tail_dword(0xAABBCCDDu, 1, 4) == 0 &&
            ds::tail_dword(0xAABBCCDDu, 1, 6) == 0x0000CCDDu && ds::tail_dword(0xAABBCCDDu, 15, 63) == 0x00BBCCDDu,
        "tail_dword");

  std::vector<Stream> set(1);
  Stream& S = set[0];
  S.length = (1ull << 35) + 40;
  for (int j = 0; j < 8; ++j) S.state[j] = 0x01234567u * (uint32_t)(j + 1);
  for (int j = 0; j < 40; ++j) S.tail[j] = (uint8_t)(j * 11 + 3);
  Round R;
  R.arena.resize(7 + 100 + kSlack);
  for (size_t i = 0; i < R.arena.size(); ++i) R.arena[i] = (uint8_t)(i * 13 + 5);
  R.off = {7, 7 + 33};
  R.len = {33, 67};
  R.begin = {0, 2};
  // the digest after the write, by the restatement
  Stream want;
  std::memcpy(want.state, S.state, 32);
  std::vector<uint8_t> msg(S.tail.get(), S.tail.get() + 40);
  msg.insert(msg.end(), R.arena.begin() + 7, R.arena.begin() + 107);
  for (size_t b = 0; b < msg.size() / 64; ++b) compress_bytes(want.state, msg.data() + 64 * b);
  std::memcpy(want.tail.get(), msg.data() + 64 * (msg.size() / 64), msg.size() % 64);
  want.length = S.length + 100;
  R.digests.resize(32);
  sum_stream(want, R.digests.data());
  R.lengths = {want.length};
  uint64_t loads = 0;
  check_round(name, set, R, &loads);
  if (!g_failed) std::printf("edges: a stream of 2^35 + 40 bytes, %llu loads ok\n", (unsigned long long)loads);
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc && !g_failed; ++i) check_file(argv[i]);
  if (!g_failed) check_edges();
  if (g_failed) return 1;
  std::printf("stream_device ok\n");
  return 0;
}
