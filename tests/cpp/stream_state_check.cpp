// The exported stream state and the id lists of mirbft_amd/csrc/stream_state.hpp as a
// stand-alone host program, built with -fsanitize=address,undefined by
// tests/test_stream_state.py, which writes the cases and the bytes it expects
// (struct.pack, nothing of the header's) into the file named on the command line.
// Every buffer handed to the header is a heap block of exactly the size its contract
// gives, so a byte read or written past it is reported. Records, little-endian:
//   'E'  state[8] u32, length u64, buf[length % 64], want[108]
//        encode gives want; decode(want) gives state, buf then zeros, length
//   'D'  dirty[108], clean[108]      decode(dirty) drops what lies past length % 64:
//        encoded again it is clean
//   'M'  blob[108], ok u8            has_magic(blob) == ok
//   'L'  has_id u8, k u64, id[k] u64 (has_id only), m u64, want[m] u64
//        last_wins(id, k) gives want
//   'V'  n u64, has_id u8, k u64, id[k] u64 (has_id only), ok u8     ids_valid
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../mirbft_amd/csrc/stream_state.hpp"

namespace ss = msha::sstate;

static FILE* g_in;
static int g_bad;

template <class T>
static std::unique_ptr<T[]> take(uint64_t n) {  // exactly n elements, from the file
  std::unique_ptr<T[]> p(new T[n]);
  if (n && std::fread(p.get(), sizeof(T), n, g_in) != n) {
    std::printf("short read\n");
    std::exit(2);
  }
  return p;
}
template <class T>
static T one() {
  return take<T>(1)[0];
}

static void fail(const char* what, uint64_t rec) {
  std::printf("MISMATCH record %" PRIu64 ": %s\n", rec, what);
  ++g_bad;
}

int main(int argc, char** argv) {
  if (argc != 2 || !(g_in = std::fopen(argv[1], "rb"))) {
    std::printf("usage: stream_state_check CASES\n");
    return 2;
  }
  uint64_t rec = 0, n_e = 0, n_d = 0, n_m = 0, n_l = 0, n_v = 0;
  for (int tag; (tag = std::fgetc(g_in)) != EOF; ++rec) {
    if (tag == 'E') {
      auto state = take<uint32_t>(8);
      const uint64_t length = one<uint64_t>();
      auto buf = take<uint8_t>(length % 64);
      auto want = take<uint8_t>(ss::kBytes);
      std::unique_ptr<uint8_t[]> got(new uint8_t[ss::kBytes]);
      std::memset(got.get(), 0xA5, ss::kBytes);
      ss::encode(state.get(), buf.get(), length, got.get());
      if (std::memcmp(got.get(), want.get(), ss::kBytes) != 0) fail("encode", rec);
      if (!ss::has_magic(got.get())) fail("magic of an encoded state", rec);
      std::unique_ptr<uint32_t[]> state2(new uint32_t[8]);
      std::unique_ptr<uint8_t[]> buf2(new uint8_t[64]);
      std::memset(buf2.get(), 0xA5, 64);
      uint64_t length2 = ~length;
      ss::decode(got.get(), state2.get(), buf2.get(), &length2);
      if (std::memcmp(state2.get(), state.get(), 32) != 0 || length2 != length) fail("decode: state or length", rec);
      if (std::memcmp(buf2.get(), buf.get(), length % 64) != 0) fail("decode: buffer", rec);
      for (uint64_t j = length % 64; j < 64; ++j)
        if (buf2[j]) fail("decode: bytes past length % 64", rec);
      ++n_e;
    } else if (tag == 'D') {
      auto dirty = take<uint8_t>(ss::kBytes);
      auto clean = take<uint8_t>(ss::kBytes);
      std::unique_ptr<uint32_t[]> state(new uint32_t[8]);
      std::unique_ptr<uint8_t[]> buf(new uint8_t[64]);
      uint64_t length = 0;
      ss::decode(dirty.get(), state.get(), buf.get(), &length);
      for (uint64_t j = length % 64; j < 64; ++j)
        if (buf[j]) fail("decode kept a byte past length % 64", rec);
      std::unique_ptr<uint8_t[]> tail(new uint8_t[length % 64]);  // only what counts goes back in
      std::memcpy(tail.get(), buf.get(), length % 64);
      std::unique_ptr<uint8_t[]> again(new uint8_t[ss::kBytes]);
      ss::encode(state.get(), tail.get(), length, again.get());
      if (std::memcmp(again.get(), clean.get(), ss::kBytes) != 0) fail("decode + encode of a dirty blob", rec);
      ++n_d;
    } else if (tag == 'M') {
      auto blob = take<uint8_t>(ss::kBytes);
      const bool ok = one<uint8_t>() != 0;
      if (ss::has_magic(blob.get()) != ok) fail("has_magic", rec);
      ++n_m;
    } else if (tag == 'L' || tag == 'V') {
      const uint64_t n = tag == 'V' ? one<uint64_t>() : 0;
      const bool has_id = one<uint8_t>() != 0;
      const uint64_t k = one<uint64_t>();
      std::unique_ptr<uint64_t[]> id;
      if (has_id) id = take<uint64_t>(k);
      if (tag == 'V') {
        const bool ok = one<uint8_t>() != 0;
        if (ss::ids_valid(n, id.get(), k) != ok) fail("ids_valid", rec);
        ++n_v;
        continue;
      }
      const uint64_t m = one<uint64_t>();
      auto want = take<uint64_t>(m);
      const std::vector<uint64_t> got = ss::last_wins(id.get(), k);
      if (got.size() != m || (m && std::memcmp(got.data(), want.get(), 8 * m) != 0)) fail("last_wins", rec);
      ++n_l;
    } else {
      std::printf("unknown record %c\n", tag);
      return 2;
    }
  }
  if (g_bad) return 1;
  std::printf("stream_state ok: %" PRIu64 " encode, %" PRIu64 " dirty, %" PRIu64 " magic, %" PRIu64
              " last_wins, %" PRIu64 " ids_valid\n",
              n_e, n_d, n_m, n_l, n_v);
  return 0;
}
