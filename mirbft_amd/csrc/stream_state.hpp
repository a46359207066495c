// The exported state of one SHA-256 stream (include/mirsha.h MSHA_STREAM_STATE_BYTES:
// crypto/sha256's MarshalBinary) and the id lists of the calls that move such states:
// shared by the stream sets (streams.cpp) and the device stream sets
// (stream_device.cpp), whose device-side row layouts stay their own. No HIP here, so the
// sanitizer test (tests/cpp/stream_state_check.cpp) compiles it alone.
//
//   bytes   0 ..   3  magic "sha\x03"
//           4 ..  35  the eight state words, big-endian
//          36 ..  99  the buffered bytes: length % 64 of them, then zeros
//         100 .. 107  length, big-endian
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

namespace msha {
namespace sstate {

constexpr uint64_t kBytes = 108;
constexpr uint8_t kMagic[4] = {'s', 'h', 'a', 0x03};

inline uint32_t be32(const uint8_t* p) {
  return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
}
inline void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v;
}

// out[0, 108) from the state words, the length % 64 buffered bytes at buf (no byte past
// them is read) and the length.
inline void encode(const uint32_t state[8], const uint8_t* buf, uint64_t length, uint8_t* out) {
  std::memcpy(out, kMagic, 4);
  for (int w = 0; w < 8; ++w) put_be32(out + 4 + 4 * w, state[w]);
  std::memset(out + 36, 0, 64);
  if (length % 64) std::memcpy(out + 36, buf, length % 64);
  put_be32(out + 100, (uint32_t)(length >> 32));
  put_be32(out + 104, (uint32_t)length);
}

// The reverse, from in[0, 108): buf[0, 64) gets the length % 64 buffered bytes, then
// zeros (what the blob holds past them is dropped). The magic is the caller's to check.
inline void decode(const uint8_t* in, uint32_t state[8], uint8_t* buf, uint64_t* length) {
  for (int w = 0; w < 8; ++w) state[w] = be32(in + 4 + 4 * w);
  *length = (uint64_t)be32(in + 100) << 32 | be32(in + 104);
  std::memset(buf, 0, 64);
  std::memcpy(buf, in + 36, *length % 64);
}

inline bool has_magic(const uint8_t* in) { return std::memcmp(in, kMagic, 4) == 0; }

// k ids that name streams of a set of n (id null: all of them, in order, so k must be n).
inline bool ids_valid(uint64_t n, const uint64_t* id, uint64_t k) {
  if (!id) return k == n;
  for (uint64_t j = 0; j < k; ++j)
    if (id[j] >= n) return false;
  return true;
}

// Sequential UnmarshalBinary over k entries: of the entries that name one stream the
// last wins. Returns the entries that take effect, in call order (id null: all k).
inline std::vector<uint64_t> last_wins(const uint64_t* id, uint64_t k) {
  std::vector<uint64_t> last(k);
  std::iota(last.begin(), last.end(), uint64_t(0));
  if (id) {
    std::vector<uint64_t> ord(last);
    std::stable_sort(ord.begin(), ord.end(), [&](uint64_t a, uint64_t b) { return id[a] < id[b]; });
    last.clear();
    for (uint64_t a = 0; a < k; ++a)
      if (a + 1 == k || id[ord[a + 1]] != id[ord[a]]) last.push_back(ord[a]);
    std::sort(last.begin(), last.end());
  }
  return last;
}

}  // namespace sstate
}  // namespace msha
