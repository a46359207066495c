// Stand-alone check of mirbft_amd/csrc/verify.hpp (tests/test_verify_cpu.py builds it
// with -fsanitize=address,undefined and runs it). The header is what k_verify_compare and
// k_verify_scan run; here a wave's 64 lanes and the scan workgroup's threads run one
// after the other, and callbacks stand in for the loads, the stores and the workgroup
// prefix.
//
// Every array is a heap block of exactly its contract size: 32 n bytes of got,
// 32 n_expected of expected, 4 n of indices, ceil(n / 64) mask words, list_cap list
// entries. So an expected row read for an out-of-range index, a store past the last
// mask word or a list entry past list_cap is an AddressSanitizer report. Beyond that the
// program checks that every mask word is stored exactly once, that no list rank is
// written twice or at or past min(bad, list_cap), and that every thread of the walk
// returns the same count.
//
// argv[1]: the cases tests/verify_matrix.py wrote (write_cases); argv[2]: where the
// results go (per case the five result words, the mask, the whole list), which the
// pytest file compares with its numpy oracle. A line a case is printed as well.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mirbft_amd/csrc/verify.hpp"

namespace mp = msha::parts;
namespace vf = msha::verify;

typedef unsigned long long ull;

static int g_failed = 0;
#define CHECK(cond, ...)                                       \
  do {                                                         \
    if (!(cond)) {                                             \
      std::printf("FAIL case %llu:%d: %s: ", (ull)k, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                \
      std::printf("\n");                                       \
      ++g_failed;                                              \
    }                                                          \
  } while (0)

static const uint32_t kListSentinel = 0xA5A5A5A5u;
static const uint32_t kFlip = 0x5A;

// tests/verify_matrix.py base_rows
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

static mp::Granule granule_at(const uint8_t* p) {
  mp::Granule g;
  std::memcpy(g.d, p, 16);
  return g;
}

static bool read_words(std::FILE* f, void* dst, uint64_t bytes) {
  const uint64_t padded = (bytes + 7u) & ~uint64_t(7);
  std::vector<uint8_t> buf(padded);
  if (padded && std::fread(buf.data(), 1, padded, f) != padded) return false;
  if (bytes) std::memcpy(dst, buf.data(), bytes);
  return true;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::printf("usage: verify_check CASES RESULTS\n");
    return 2;
  }
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  uint64_t count = 0;
  if (!in || !out || std::fread(&count, 8, 1, in) != 1) {
    std::printf("cannot open the case or the result file\n");
    return 2;
  }
  for (uint64_t k = 0; k < count; ++k) {
    uint64_t h[6];
    if (std::fread(h, 8, 6, in) != 6) return 2;
    const uint64_t n = h[0], n_expected = h[1], list_cap = h[3], n_flips = h[4];
    const bool has_idx = h[2] != 0;
    const uint64_t words = vf::mask_words(n);

    uint32_t* const idx = has_idx ? exact<uint32_t>(n) : nullptr;
    if (has_idx && !read_words(in, idx, 4 * n)) return 2;
    std::vector<uint32_t> flips(3 * n_flips);
    if (!read_words(in, flips.data(), 12 * n_flips)) return 2;

    uint8_t* const got = exact<uint8_t>(32 * n);
    uint8_t* const expected = exact<uint8_t>(32 * n_expected);
    for (uint64_t e = 0; e < n_expected; ++e) base_row(e, expected + 32 * e);
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t e = has_idx ? idx[i] : i;
      base_row(e < n_expected ? e : i, got + 32 * i);
    }
    for (uint64_t j = 0; j < n_flips; ++j)
      (flips[3 * j] == 0 ? got : expected)[32ull * flips[3 * j + 1] + flips[3 * j + 2]] ^= kFlip;

    uint64_t* const mask = exact<uint64_t>(words);
    std::memset(mask, 0xFF, 8 * words);
    uint32_t* const list = exact<uint32_t>(list_cap);
    for (uint64_t j = 0; j < list_cap; ++j) list[j] = kListSentinel;

    // k_verify_compare: workgroups of kCompareThreads lanes over whole words, a wave a word
    std::vector<uint8_t> stored(words, 0);
    const uint64_t waves = (n + vf::kCompareThreads - 1) / vf::kCompareThreads * (vf::kCompareThreads / 64);
    for (uint64_t wv = 0; wv < waves; ++wv) {
      uint64_t ballot = 0;
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint64_t i = wv * 64 + lane;
        bool d = false;
        if (i < n)
          d = vf::differs(
              i, n_expected, has_idx, [&](uint64_t s) { return idx[s]; },
              [&](uint64_t s, uint32_t half) { return granule_at(got + 32 * s + 16 * half); },
              [&](uint64_t e, uint32_t half) { return granule_at(expected + 32 * e + 16 * half); });
        if (d) ballot |= uint64_t(1) << lane;
      }
      const uint64_t w = vf::word_of(wv * 64);
      if (w < vf::mask_words(n)) {
        mask[w] = ballot & vf::valid_bits(w, n);
        stored[w]++;
      }
    }
    for (uint64_t w = 0; w < words; ++w) CHECK(stored[w] == 1, "mask word %llu stored %d times", (ull)w, stored[w]);

    // k_verify_scan: the workgroup prefix of each chunk, then every thread's walk
    const uint64_t chunks = (words + vf::kScanWords - 1) / vf::kScanWords;
    std::vector<uint32_t> before(chunks * vf::kScanThreads), all(chunks);
    for (uint64_t c = 0; c < chunks; ++c) {
      uint32_t sum = 0;
      for (uint32_t t = 0; t < vf::kScanThreads; ++t) {
        before[c * vf::kScanThreads + t] = sum;
        const uint64_t w = c * vf::kScanWords + t;
        if (w < words) sum += (uint32_t)__builtin_popcountll(mask[w]);
      }
      all[c] = sum;
    }
    std::vector<uint8_t> written(list_cap, 0);
    uint64_t bad = 0, first = vf::kNone, bad_index = 0, total_bits = 0;
    for (uint64_t c = 0; c < chunks; ++c) total_bits += all[c];
    const uint64_t limit = total_bits < list_cap ? total_bits : list_cap;
    for (uint32_t t = 0; t < vf::kScanThreads; ++t) {
      uint64_t chunk = 0;
      vf::Seen seen;
      const uint64_t b = vf::walk(
          words, t, list_cap, has_idx, [&](uint64_t w) { return mask[w]; },
          [&](uint32_t cnt, uint32_t* bf, uint32_t* al) {
            const uint64_t w = chunk * vf::kScanWords + t;
            CHECK(cnt == (w < words ? (uint32_t)__builtin_popcountll(mask[w]) : 0u), "thread %u chunk %llu counts %u", t,
                  (ull)chunk, cnt);
            *bf = before[chunk * vf::kScanThreads + t];
            *al = all[chunk];
            ++chunk;
          },
          [&](uint64_t r, uint32_t slot) {
            if (r >= limit) {  // not performed: the contract is already broken
              CHECK(r < limit, "rank %llu written, min(bad, list_cap) is %llu", (ull)r, (ull)limit);
              return;
            }
            CHECK(written[r] == 0, "rank %llu written twice", (ull)r);
            written[r] = 1;
            list[r] = slot;
          },
          [&](uint64_t slot) { return (uint64_t)idx[slot] >= n_expected; }, &seen);
      CHECK(chunk == chunks, "thread %u asked for %llu prefixes, the walk has %llu chunks", t, (ull)chunk, (ull)chunks);
      if (t == 0) bad = b;
      CHECK(b == bad, "thread %u counts %llu set bits, thread 0 %llu", t, (ull)b, (ull)bad);
      first = seen.first < first ? seen.first : first;
      bad_index += seen.bad_index;
    }
    uint64_t r[5];
    vf::result_words(n, bad, first, list_cap, bad_index, r);
    std::printf("case %llu: n %llu bad %llu first_bad %llu listed %llu bad_index %llu\n", (ull)k, (ull)r[0], (ull)r[1],
                (ull)r[2], (ull)r[3], (ull)r[4]);

    std::fwrite(r, 8, 5, out);
    std::fwrite(mask, 8, words, out);
    std::fwrite(list, 4, list_cap, out);
    if (list_cap & 1u) {
      const uint32_t pad = 0;
      std::fwrite(&pad, 4, 1, out);
    }
    std::free(idx);
    std::free(got);
    std::free(expected);
    std::free(mask);
    std::free(list);
  }
  std::fclose(in);
  std::fclose(out);
  if (g_failed) {
    std::printf("verify FAILED: %d checks\n", g_failed);
    return 1;
  }
  std::printf("verify ok: %llu cases\n", (ull)count);
  return 0;
}
