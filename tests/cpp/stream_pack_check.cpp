// Stand-alone check of mirbft_amd/csrc/stream_pack.hpp (tests/test_streams_pack.py
// builds it with -fsanitize=address,undefined and runs it): plans writes over edge
// and random inputs, replays every emitted copy into exactly sized buffers (so a
// copy out of bounds is a sanitizer error as well as a failed check), and checks
// per stream that the staged blocks followed by the new tail are the old tail
// followed by the chunks.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../mirbft_amd/csrc/stream_pack.hpp"

namespace sp = msha::spack;

static int g_failed = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::printf("FAIL %s:%d: %s: ", name, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
      ++g_failed;                                         \
      return;                                             \
    }                                                     \
  } while (0)

struct Set {
  uint64_t n;
  std::vector<uint64_t> length;
  std::vector<uint8_t> tail;  // 64 n
  std::vector<std::vector<uint8_t>> all;  // everything written, per stream (the model)
};

// One write: plan, replay, check, commit. Returns the plan's piece count through *pieces.
static void write_case(const char* name, Set& S, const std::vector<uint8_t>& arena, const std::vector<uint64_t>& id,
                       const std::vector<uint64_t>& off, const std::vector<uint64_t>& len, uint64_t staging,
                       uint64_t* pieces = nullptr, uint64_t* max_piece = nullptr) {
  const uint64_t k = id.size();
  CHECK(sp::valid(S.n, arena.size(), id.data(), off.data(), len.data(), k), "inputs of the case");
  const uint64_t bound = sp::staging_bound(staging);
  const sp::Plan P = sp::plan(S.length.data(), id.data(), off.data(), len.data(), k, staging);
  if (pieces) *pieces = P.pieces.size();
  // the model: old tail + chunks, per touched stream
  std::map<uint64_t, std::vector<uint8_t>> want;
  uint64_t bytes = 0;
  for (uint64_t j = 0; j < k; ++j) {
    auto it = want.find(id[j]);
    if (it == want.end()) {
      const uint64_t t = S.length[id[j]] % 64;
      it = want.emplace(id[j], std::vector<uint8_t>(S.tail.begin() + 64 * id[j], S.tail.begin() + 64 * id[j] + t)).first;
    }
    it->second.insert(it->second.end(), arena.begin() + off[j], arena.begin() + off[j] + len[j]);
    S.all[id[j]].insert(S.all[id[j]].end(), arena.begin() + off[j], arena.begin() + off[j] + len[j]);
    bytes += len[j];
  }
  CHECK(P.bytes == bytes, "%llu != %llu", (unsigned long long)P.bytes, (unsigned long long)bytes);
  CHECK(P.slots == want.size(), "one scratch slot per touched stream");
  std::vector<uint8_t> new_tail(64 * P.slots, 0xEE);
  std::map<uint64_t, std::vector<uint8_t>> got;  // staged blocks per stream, in piece order
  std::map<uint64_t, uint64_t> got_blocks;
  std::map<uint64_t, sp::Commit> last;
  auto replay = [&](const sp::Copy& c, std::vector<uint8_t>* staging_buf) -> bool {
    const uint8_t* src;
    if (c.src_space == sp::kArena) {
      if (c.src > arena.size() || c.len > arena.size() - c.src) return false;
      src = arena.data() + c.src;
    } else if (c.src_space == sp::kOldTail) {
      const uint64_t s = c.src / 64, pos = c.src % 64;
      if (s >= S.n || pos + c.len > S.length[s] % 64) return false;
      src = S.tail.data() + c.src;
    } else {
      return false;
    }
    uint8_t* dst;
    if (c.dst_space == sp::kStaging) {
      if (!staging_buf || c.dst > staging_buf->size() || c.len > staging_buf->size() - c.dst) return false;
      dst = staging_buf->data() + c.dst;
    } else if (c.dst_space == sp::kNewTail) {
      if (c.dst / 64 >= P.slots || c.dst % 64 + c.len > 63) return false;
      dst = new_tail.data() + c.dst;
    } else {
      return false;
    }
    if (c.len) std::memcpy(dst, src, c.len);
    return true;
  };
  uint64_t blocks = 0;
  for (const sp::Piece& p : P.pieces) {
    CHECK(p.bytes <= bound && p.bytes % 64 == 0 && p.bytes == 64 * p.blocks, "piece of %llu bytes, bound %llu",
          (unsigned long long)p.bytes, (unsigned long long)bound);
    if (max_piece && p.bytes > *max_piece) *max_piece = p.bytes;
    CHECK(!p.lanes.empty() && p.lanes.size() == p.commits.size(), "a commit per lane");
    std::vector<uint8_t> st(p.bytes, 0xDD);  // exactly the piece: an overrun is an ASan error
    for (const sp::Copy& c : p.copies) CHECK(replay(c, &st), "copy out of bounds");
    uint64_t sum = 0;
    std::map<uint64_t, int> seen;
    for (size_t l = 0; l < p.lanes.size(); ++l) {
      const sp::Lane& ln = p.lanes[l];
      CHECK(ln.nblocks >= 1 && ln.off % 64 == 0 && ln.off + 64 * ln.nblocks <= p.bytes, "lane range");
      CHECK(l == 0 || p.lanes[l - 1].nblocks >= ln.nblocks, "lanes in descending block count");
      CHECK(seen[ln.id]++ == 0, "one lane a stream in a piece");
      CHECK(p.commits[l].id == ln.id, "commit order");
      got[ln.id].insert(got[ln.id].end(), st.begin() + ln.off, st.begin() + ln.off + 64 * ln.nblocks);
      got_blocks[ln.id] += ln.nblocks;
      last[ln.id] = p.commits[l];
      // a stream whose run goes on sits at a block boundary with no tail
      if (p.commits[l].slot == sp::kNoSlot) CHECK(p.commits[l].length % 64 == 0 && p.commits[l].tail_len == 0, "mid-run commit");
      sum += ln.nblocks;
    }
    CHECK(sum == p.blocks, "piece block count");
    blocks += sum;
  }
  CHECK(blocks == P.blocks, "plan block count");
  for (const sp::Copy& c : P.host_copies) CHECK(replay(c, nullptr), "host copy out of bounds");
  for (const sp::Commit& c : P.host_commits) {
    CHECK(!last.count(c.id) && !got.count(c.id), "a host-only stream has no lane");
    last[c.id] = c;
  }
  CHECK(last.size() == want.size(), "every touched stream is committed");
  for (auto& kv : want) {
    const uint64_t s = kv.first;
    const std::vector<uint8_t>& w = kv.second;
    const sp::Commit& c = last[s];
    CHECK(c.slot != sp::kNoSlot && c.slot < P.slots, "final commit installs a tail");
    CHECK(got_blocks[s] == w.size() / 64, "stream %llu: %llu blocks, want %llu", (unsigned long long)s,
          (unsigned long long)got_blocks[s], (unsigned long long)(w.size() / 64));
    CHECK(c.tail_len == w.size() % 64, "tail length");
    std::vector<uint8_t> cat = got[s];
    cat.insert(cat.end(), new_tail.begin() + 64 * c.slot, new_tail.begin() + 64 * c.slot + c.tail_len);
    CHECK(cat == w, "stream %llu: staged blocks + new tail differ from old tail + chunks", (unsigned long long)s);
    CHECK(c.length == S.all[s].size(), "new length");
    // commit
    S.length[s] = c.length;
    std::memset(&S.tail[64 * s], 0, 64);
    std::memcpy(&S.tail[64 * s], &new_tail[64 * c.slot], c.tail_len);
    CHECK(c.tail_len == 0 || std::memcmp(&S.tail[64 * s],S.all[s].data() + S.all[s].size() - c.tail_len, c.tail_len) == 0, "tail bytes");
  }
}

static Set make_set(uint64_t n) {
  Set S;
  S.n = n;
  S.length.assign(n, 0);
  S.tail.assign(64 * n, 0);
  S.all.resize(n);
  return S;
}

static std::vector<uint8_t> random_bytes(std::mt19937_64& g, uint64_t n) {
  std::vector<uint8_t> a(n);
  for (auto& b : a) b = (uint8_t)g();
  return a;
}

static void cases() {
  std::mt19937_64 g(20240607);
  const char* name = "cases";
  {  // k = 0
    Set S = make_set(3);
    uint64_t pieces = 9;
    write_case("k0", S, {}, {}, {}, {}, 0, &pieces);
    CHECK(pieces == 0, "k = 0 plans nothing");
  }
  {  // zero-length chunks, alone and between others
    Set S = make_set(4);
    const auto a = random_bytes(g, 300);
    write_case("zero_len", S, a, {0, 1, 1, 1, 2}, {0, 10, 10, 20, 300}, {0, 100, 0, 30, 0}, 4096);
    write_case("zero_len2", S, a, {1, 3}, {0, 0}, {0, 0}, 4096);
  }
  {  // every id the same: 50 chunks of mixed sizes on one stream
    Set S = make_set(2);
    const auto a = random_bytes(g, 5000);
    std::vector<uint64_t> id(50, 1), off, len;
    uint64_t pos = 0;
    for (int j = 0; j < 50; ++j) {
      const uint64_t l = (uint64_t)(g() % 200);
      off.push_back(pos);
      len.push_back(l);
      pos += l / 2;  // overlapping ranges are fine
    }
    write_case("same_id", S, a, id, off, len, 4096);
  }
  {  // tail 63 plus 1 byte
    Set S = make_set(1);
    const auto a = random_bytes(g, 128);
    uint64_t pieces = 0;
    write_case("tail63", S, a, {0}, {0}, {63}, 4096, &pieces);
    CHECK(pieces == 0 && S.length[0] == 63, "63 bytes stay on the host");
    write_case("tail63+1", S, a, {0}, {63}, {1}, 4096, &pieces);
    CHECK(pieces == 1 && S.length[0] == 64, "the 64th byte completes a block");
  }
  {  // a run that exactly fills a piece, then one block more
    Set S = make_set(2);
    const auto a = random_bytes(g, 8192);
    uint64_t pieces = 0, mx = 0;
    write_case("exact_piece", S, a, {0}, {0}, {4096}, 4096, &pieces, &mx);
    CHECK(pieces == 1 && mx == 4096, "4096 bytes are one full piece (got %llu)", (unsigned long long)pieces);
    write_case("piece_plus_block", S, a, {1}, {0}, {4096 + 64}, 4096, &pieces);
    CHECK(pieces == 2, "one block over the bound is a second piece");
  }
  {  // a run that spans 3 pieces at staging_bytes = 4096, with other streams beside it
    Set S = make_set(5);
    const auto a = random_bytes(g, 12000);
    uint64_t pieces = 0;
    write_case("warm", S, a, {0, 2, 4}, {0, 7, 9}, {17, 63, 1}, 4096);
    write_case("span3", S, a, {1, 0, 2, 3, 4, 0}, {0, 100, 200, 300, 400, 500}, {10000, 130, 1, 700, 64, 31}, 4096, &pieces);
    CHECK(pieces >= 3, "10,000 bytes at 4,096 a piece span 3 pieces (got %llu)", (unsigned long long)pieces);
  }
  {  // staging_bound
    CHECK(sp::staging_bound(0) == (64ull << 20) && sp::staging_bound(1) == 4096 && sp::staging_bound(5000) == 4992,
          "staging_bound");
    const uint64_t id1[] = {3}, off1[] = {0}, len1[] = {1}, off2[] = {~0ull}, len2[] = {2};
    const uint64_t id0[] = {0};
    CHECK(!sp::valid(3, 10, id1, off1, len1, 1), "id == n is invalid");
    CHECK(!sp::valid(3, 10, id0, off2, len2, 1), "offset overflow is invalid");
    const uint64_t off3[] = {9};
    CHECK(!sp::valid(3, 10, id0, off3, len2, 1) && sp::valid(3, 10, id0, off3, len1, 1), "range end");
  }
  // random rounds on one set: state carries over between writes
  for (int trial = 0; trial < 40; ++trial) {
    const uint64_t n = 1 + g() % 40;
    Set S = make_set(n);
    const uint64_t staging = (g() % 3 == 0) ? 4096 : (g() % 2 ? 8192 : 64 * (64 + g() % 200));
    for (int round = 0; round < 6; ++round) {
      const auto a = random_bytes(g, 1 + g() % 20000);
      const uint64_t k = g() % 60;
      std::vector<uint64_t> id, off, len;
      for (uint64_t j = 0; j < k; ++j) {
        id.push_back(g() % n);
        const uint64_t o = g() % (a.size() + 1);
        const uint64_t room = a.size() - o;
        uint64_t l;
        switch (g() % 5) {
          case 0: l = 0; break;
          case 1: l = g() % 65; break;
          case 2: l = 64 * (g() % 4); break;
          default: l = g() % (room + 1); break;
        }
        off.push_back(o);
        len.push_back(l > room ? room : l);
      }
      write_case("random", S, a, id, off, len, staging);
      if (g_failed) break;
    }
    if (g_failed) break;
  }
}

int main() {
  cases();
  if (g_failed) {
    std::printf("%d check(s) failed\n", g_failed);
    return 1;
  }
  std::printf("stream_pack ok\n");
  return 0;
}
