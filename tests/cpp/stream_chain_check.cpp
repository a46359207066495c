// The host-checkable decisions of the eight-lane absorb chain and of
// msha_dstreams_write_routed_device (mirbft_amd/csrc/stream_chain.hpp), as a stand-alone
// program for AddressSanitizer + UBSan (tests/test_dstream_route_cpu.py builds and runs
// it):
//   barriers  for NB in 0..200 under both per values, the producers' and the consumers'
//             barrier calls are equal in number and carry the same ids in the same
//             order; every block is scheduled by exactly one producer into the slot the
//             consumers read it from; no prefetch goes past a lane's last block;
//   long      whole_blocks / is_long_row over t in 0..63 against sums around
//             64 long_blocks - t, and at the top of the 64-bit range, against 128-bit
//             arithmetic;
//   tail      the new tail row of a routed stream, built as k_sroute_tail builds it from
//             a message held in an allocation of exactly round16(total) bytes, against
//             the bytes themselves;
//   length    new_length wraps as hash.Hash's count does, with no signed arithmetic;
//   layout    the workspace's offsets at the count bounds: ordered, aligned, in 64 bits.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mirbft_amd/csrc/stream_chain.hpp"

namespace sc = msha::schain;
typedef unsigned __int128 u128;

static int failures = 0;
#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      ++failures;                         \
      std::printf("FAIL %s: ", #cond);    \
      std::printf(__VA_ARGS__);           \
      std::printf("\n");                  \
    }                                     \
  } while (0)

// The barrier ids of a producer wave, by the kernel's loop.
static std::vector<uint32_t> producer_ids(uint32_t NB, uint32_t per, uint32_t pw, std::vector<int>* owner,
                                          std::vector<uint32_t>* slot) {
  std::vector<uint32_t> ids;
  for (uint32_t b = 0; b < NB; ++b) {
    if (sc::producer_of(b) == pw) {
      (*owner)[b] += 1;
      (*slot)[b] = 2 * sc::slot_of(b, per) + sc::sub_of(b, per);
    }
    if (sc::producer_barrier_after(b, NB, per)) ids.push_back(b / per);
  }
  ids.push_back(sc::groups(NB, per));
  return ids;
}

// The barrier ids of a consumer wave and the slot it reads each block's K+W from.
static std::vector<uint32_t> consumer_ids(uint32_t NB, uint32_t per, std::vector<uint32_t>* read_slot) {
  std::vector<uint32_t> ids;
  ids.push_back(0);
  if (per == 2) {
    const uint32_t NP = sc::groups(NB, 2);
    for (uint32_t g = 0; g < NP; ++g) {
      ids.push_back(g + 1);
      // group g's blocks were read from slot g & 1 during group g - 1 (group 0: after barrier 0)
      if (2 * g < NB) (*read_slot)[2 * g] = 2 * (g & 1);
      if (2 * g + 1 < NB) (*read_slot)[2 * g + 1] = 2 * (g & 1) + 1;
    }
    return ids;
  }
  for (uint32_t b = 0; b < NB; ++b) {
    ids.push_back(b + 1);
    (*read_slot)[b] = 2 * (b & 1);
  }
  return ids;
}

static void check_barriers() {
  for (uint32_t per = 1; per <= 2; ++per) {
    for (uint32_t NB = 0; NB <= 200; ++NB) {
      std::vector<int> owner(NB, 0);
      std::vector<uint32_t> wslot(NB, 99), rslot(NB, 98);
      const std::vector<uint32_t> p0 = producer_ids(NB, per, 0, &owner, &wslot);
      const std::vector<uint32_t> p1 = producer_ids(NB, per, 1, &owner, &wslot);
      const std::vector<uint32_t> c = consumer_ids(NB, per, &rslot);
      CHECK(p0 == p1, "NB %u per %u: the producers differ", NB, per);
      CHECK(p0 == c, "NB %u per %u: producers make %zu barrier calls, consumers %zu", NB, per, p0.size(), c.size());
      CHECK(p0.size() == (size_t)sc::groups(NB, per) + 1, "NB %u per %u", NB, per);
      if (NB) {
        CHECK(sc::producer_barrier_calls(NB, per) == p0.size(), "NB %u per %u", NB, per);
        CHECK(sc::consumer_barrier_calls(NB, per) == c.size(), "NB %u per %u", NB, per);
      }
      for (size_t k = 0; k < p0.size(); ++k) CHECK(p0[k] == k, "NB %u per %u: barrier %zu has id %u", NB, per, k, p0[k]);
      for (uint32_t b = 0; b < NB; ++b) {
        CHECK(owner[b] == 1, "NB %u per %u: block %u has %d producers", NB, per, b, owner[b]);
        CHECK(wslot[b] == rslot[b], "NB %u per %u: block %u written to %u, read from %u", NB, per, b, wslot[b], rslot[b]);
      }
    }
  }
  for (uint32_t NB = 0; NB <= 200; ++NB) {
    CHECK(sc::per_for(NB, 2) == (NB >= 64 ? 2u : 1u), "NB %u", NB);
    CHECK(sc::per_for(NB, 1) == 1u, "NB %u", NB);
  }
  CHECK(sc::groups(0xFFFFFFFEu, 2) == 0x7FFFFFFFu && sc::groups(0xFFFFFFFEu, 1) == 0xFFFFFFFEu, "groups at the top");
  // a lane of nb blocks: the loads a producer issues are exactly its own blocks below nb
  for (uint32_t nb = 0; nb <= 9; ++nb)
    for (uint32_t NB = nb; NB <= 12; ++NB)
      for (uint32_t pw = 0; pw < sc::kProducers; ++pw) {
        std::vector<int> loaded(NB + sc::kProducers + 1, 0);
        if (sc::prefetch_ok(pw, nb)) loaded[pw]++;
        for (uint32_t b = 0; b < NB; ++b)
          if (sc::producer_of(b) == pw && sc::prefetch_ok(b + sc::kProducers, nb)) loaded[b + sc::kProducers]++;
        for (uint32_t b = 0; b < loaded.size(); ++b)
          CHECK(loaded[b] == (b < nb && sc::producer_of(b) == pw ? 1 : 0), "nb %u NB %u pw %u block %u loaded %d times",
                nb, NB, pw, b, loaded[b]);
      }
}

static uint64_t check_long() {
  uint64_t n = 0;
  const uint32_t Ls[] = {1, 2, 3, 4, 64, 65, 1000, 0xFFFFFFFFu};
  for (uint32_t L : Ls)
    for (uint32_t t = 0; t < 64; ++t)
      for (int64_t d = -66; d <= 66; ++d) {
        const int64_t s = 64 * (int64_t)L - (int64_t)t + d;
        if (s < 0) continue;
        const uint64_t sum = (uint64_t)s;
        const u128 whole = ((u128)t + sum) / 64;
        CHECK(sc::whole_blocks(t, sum) == (uint64_t)whole, "t %u sum %llu", t, (unsigned long long)sum);
        CHECK(sc::new_tail(t, sum) == (uint32_t)(((u128)t + sum) % 64), "t %u sum %llu", t, (unsigned long long)sum);
        CHECK(sc::is_long_row(t, sum, L) == (whole >= L), "t %u sum %llu L %u", t, (unsigned long long)sum, L);
        CHECK(sc::message_len(t, sum) == t + sum, "t %u sum %llu", t, (unsigned long long)sum);
        CHECK(sc::tail_bytes(sc::message_len(t, sum), sc::whole_blocks(t, sum)) == sc::new_tail(t, sum), "t %u sum %llu",
              t, (unsigned long long)sum);
        ++n;
      }
  // the top of the range: nothing wraps, and such a sum is never routed
  const uint64_t top = ~0ull;
  for (uint32_t t = 0; t < 64; ++t)
    for (uint64_t sum : {top, top - 1, top - 63, top - 64, sc::kMaxSum + 1, sc::kMaxSum}) {
      CHECK(sc::whole_blocks(t, sum) == (uint64_t)(((u128)t + sum) / 64 & top), "t %u sum %llu", t, (unsigned long long)sum);
      CHECK(sc::is_long_row(t, sum, 1) == (sum <= sc::kMaxSum), "t %u sum %llu", t, (unsigned long long)sum);
      ++n;
    }
  return n;
}

static uint64_t check_tail() {
  uint64_t n = 0;
  for (uint64_t total = 64; total <= 64 * 5 + 63; ++total) {
    const uint64_t whole = total / 64, r16 = msha::parts_concat::round16(total);
    // the message as the copy leaves it: total bytes, the pad to 16 zeroed, nothing behind it
    uint8_t* msg = static_cast<uint8_t*>(std::malloc(r16));
    for (uint64_t i = 0; i < r16; ++i) msg[i] = i < total ? (uint8_t)(1 + (i * 37 + total) % 255) : 0;
    const uint32_t rem = sc::tail_bytes(total, whole);
    uint32_t d[16];
    for (uint32_t g = 0; g < 4; ++g) {
      uint32_t v[4] = {0, 0, 0, 0};
      if (sc::tail_granule_read(g, rem)) std::memcpy(v, msg + 64 * whole + 16 * g, 16);  // ASan: inside the message
      for (uint32_t j = 0; j < 4; ++j) d[4 * g + j] = sc::tail_row_dword(v[j], 4 * g + j, rem);
    }
    uint8_t row[64], want[64];
    std::memcpy(row, d, 64);
    std::memset(want, 0, 64);
    std::memcpy(want, msg + 64 * whole, rem);
    CHECK(std::memcmp(row, want, 64) == 0, "total %llu", (unsigned long long)total);
    CHECK(rem == total % 64, "total %llu", (unsigned long long)total);
    // bytes past rem are zero whatever lies in the granule behind them
    for (uint32_t j = 0; j < 16; ++j) {
      const uint32_t x = sc::tail_row_dword(0xFFFFFFFFu, j, rem);
      const int k = (int)rem - 4 * (int)j;
      const uint32_t wantx = k >= 4 ? 0xFFFFFFFFu : k <= 0 ? 0u : (0xFFFFFFFFu >> (8 * (4 - k)));
      CHECK(x == wantx, "rem %u dword %u", rem, j);
    }
    std::free(msg);
    ++n;
  }
  return n;
}

static void check_length() {
  CHECK(sc::new_length(0, 0) == 0, "0");
  CHECK(sc::new_length(~0ull, 1) == 0, "wraps to 0");
  CHECK(sc::new_length(~0ull - 5, 70) == 64, "wraps");
  CHECK(sc::new_length(1ull << 63, 1ull << 62) == (3ull << 62), "large");
}

static void check_layout() {
  struct B { uint64_t rows, m, flat; };
  const B bounds[] = {{1, 1, 80}, {0xFFFFFFFEull, 1, 80}, {1, 0xFFFFFFFFull, 1ull << 48},
                      {0xFFFFFFFEull, 0xFFFFFFFFull, 1ull << 48}, {65536, 4096, 32ull << 20}};
  for (const B& b : bounds) {
    const sc::Layout l(b.rows, b.m, b.flat);
    CHECK(l.ok, "rows %llu m %llu", (unsigned long long)b.rows, (unsigned long long)b.m);
    const uint64_t at[] = {l.claim, l.taken, l.slot_row, l.slot_stream, l.slot_t, l.msg_off, l.msg_len, l.blocks, l.flat, l.bytes};
    const u128 need[] = {8 * msha::parts_route::kClaimWords, b.rows, (u128)4 * b.m, (u128)4 * b.m, (u128)4 * b.m,
                         (u128)8 * b.m, (u128)8 * b.m, (u128)8 * b.m, b.flat};
    for (int k = 0; k < 9; ++k) {
      CHECK(at[k] % 64 == 0, "array %d is not 64-byte aligned", k);
      CHECK((u128)at[k] + need[k] <= (u128)at[k + 1], "array %d overlaps the next", k);
    }
    CHECK(l.flat % 256 == 0, "the flatten buffer is 256-byte aligned");
    CHECK(l.bytes == l.flat + b.flat, "bytes");
    CHECK(l.bytes < (1ull << 50), "the size stays far below 2^64");
  }
  CHECK(!sc::Layout(1ull << 32, 1, 80).ok, "rows at 2^32");
  CHECK(!sc::Layout(1, 1ull << 32, 80).ok, "slots at 2^32");
  CHECK(!sc::Layout(1, 1, (1ull << 48) + 1).ok, "flat above 2^48");
}

int main() {
  check_barriers();
  const uint64_t n_long = check_long();
  const uint64_t n_tail = check_tail();
  check_length();
  check_layout();
  if (failures) {
    std::printf("stream_chain FAILED: %d\n", failures);
    return 1;
  }
  std::printf("stream_chain ok: 402 barrier schedules, %llu decisions, %llu tails\n", (unsigned long long)n_long,
              (unsigned long long)n_tail);
  return 0;
}
