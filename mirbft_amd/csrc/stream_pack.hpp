// Host-side planning of one write to a stream set (streams.cpp): no HIP here, so
// the sanitizer test (tests/test_streams_pack.py) compiles it alone.
//
// A stream's logical input is its buffered tail (< 64 bytes) followed by its
// chunks of the call, in call order. The whole 64-byte blocks of that input go to
// the GPU; what is left becomes the new tail. plan() turns (tail lengths, jobs,
// staging bound) into
//   pieces   each at most staging_bytes of pinned staging: the copies that fill
//            it (whole blocks at 64-aligned offsets), its lane jobs in descending
//            block count (one lane a stream) and, per lane, what to commit once
//            the piece's launch has completed;
//   host     the streams the call leaves under one block: copies into their new
//            tails only, nothing to launch.
// A stream's run of blocks may end a piece and go on in the next: the chaining
// state on the device carries it over, and the commit of the first piece leaves
// the stream at a block boundary with an empty tail.
// New tails are written to scratch slots (64 bytes a touched stream), never into
// the old tails the copies still read; a commit installs a slot.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

namespace msha {
namespace spack {

constexpr uint64_t kBlock = 64;
constexpr uint64_t kMinStaging = 4096;
constexpr uint64_t kDefaultStaging = 64ull << 20;

// staging_bytes as a set uses it: 0 -> 64 MiB, at least 4096, a multiple of 64.
inline uint64_t staging_bound(uint64_t staging_bytes) {
  if (staging_bytes == 0) staging_bytes = kDefaultStaging;
  staging_bytes = std::max(staging_bytes, kMinStaging);
  return staging_bytes / kBlock * kBlock;  // (rounded down: the bound is never exceeded)
}

// Every id below n and every range inside the arena (no overflow).
inline bool valid(uint64_t n, uint64_t arena_len, const uint64_t* id, const uint64_t* off, const uint64_t* len,
                  uint64_t k) {
  for (uint64_t j = 0; j < k; ++j) {
    if (id[j] >= n) return false;
    if (off[j] > arena_len || len[j] > arena_len - off[j]) return false;
  }
  return true;
}

enum Space : uint8_t { kArena = 0, kOldTail = 1, kStaging = 2, kNewTail = 3 };

// len bytes from src (kArena: arena offset; kOldTail: 64 id + position) to dst
// (kStaging: offset in the piece's staging; kNewTail: 64 slot + position).
struct Copy {
  uint8_t src_space, dst_space;
  uint64_t src, dst, len;
};

struct Lane {
  uint64_t id;       // stream (state row)
  uint64_t off;      // staging offset of its blocks, a multiple of 64
  uint64_t nblocks;  // >= 1
};

// After the piece (or, for a host-only stream, the call): the stream's byte count
// and tail. slot == kNoSlot: an empty tail (the run goes on in the next piece).
constexpr uint64_t kNoSlot = ~0ull;
struct Commit {
  uint64_t id;
  uint64_t length;
  uint64_t slot;
  uint32_t tail_len;
};

struct Piece {
  std::vector<Copy> copies;
  std::vector<Lane> lanes;      // descending nblocks
  std::vector<Commit> commits;  // one a lane
  uint64_t bytes = 0;           // staging used, <= the bound
  uint64_t blocks = 0;
};

struct Plan {
  std::vector<Piece> pieces;
  std::vector<Copy> host_copies;  // streams left under one block
  std::vector<Commit> host_commits;
  uint64_t slots = 0;             // new-tail scratch slots used
  uint64_t bytes = 0;             // sum of the jobs' lengths
  uint64_t blocks = 0;            // blocks over all pieces
};

// tail_len[s] = length[s] % 64 for every stream of the set; the jobs are valid().
inline Plan plan(const uint64_t* length, const uint64_t* id, const uint64_t* off, const uint64_t* len, uint64_t k,
                 uint64_t staging_bytes) {
  Plan P;
  const uint64_t cap = staging_bound(staging_bytes) / kBlock;  // blocks a piece
  // jobs grouped by stream, stably
  std::vector<uint64_t> jobs(k);
  std::iota(jobs.begin(), jobs.end(), uint64_t(0));
  std::stable_sort(jobs.begin(), jobs.end(), [&](uint64_t a, uint64_t b) { return id[a] < id[b]; });
  struct Run {
    uint64_t id, j0, j1;   // jobs[j0, j1)
    uint64_t total;        // tail + chunks
  };
  std::vector<Run> runs;
  for (uint64_t a = 0; a < k;) {
    uint64_t b = a, sum = 0;
    while (b < k && id[jobs[b]] == id[jobs[a]]) sum += len[jobs[b++]];
    const uint64_t s = id[jobs[a]];
    runs.push_back(Run{s, a, b, length[s] % kBlock + sum});
    P.bytes += sum;
    a = b;
  }
  // the streams with whole blocks first, longest run first (stable: by id within a count)
  std::stable_sort(runs.begin(), runs.end(),
                   [](const Run& a, const Run& b) { return a.total / kBlock > b.total / kBlock; });

  Piece cur;
  auto close_piece = [&] {
    if (cur.lanes.empty()) return;
    // a run continued from the piece before may be shorter than the lanes after it
    std::vector<uint64_t> ord(cur.lanes.size());
    std::iota(ord.begin(), ord.end(), uint64_t(0));
    std::stable_sort(ord.begin(), ord.end(),
                     [&](uint64_t a, uint64_t b) { return cur.lanes[a].nblocks > cur.lanes[b].nblocks; });
    Piece p;
    p.copies.swap(cur.copies);
    for (uint64_t o : ord) {
      p.lanes.push_back(cur.lanes[o]);
      p.commits.push_back(cur.commits[o]);
    }
    p.bytes = cur.bytes;
    p.blocks = cur.blocks;
    P.blocks += p.blocks;
    P.pieces.push_back(std::move(p));
    cur = Piece();
  };

  for (const Run& r : runs) {
    const uint64_t s = r.id;
    const uint64_t told = length[s] % kBlock;
    const uint64_t nb = r.total / kBlock;
    const uint32_t tnew = (uint32_t)(r.total % kBlock);
    const uint64_t slot = P.slots++;
    // a cursor over the logical input: segment -1 is the old tail, then the chunks
    uint64_t seg = r.j0, segpos = 0;  // within the chunks
    uint64_t tailpos = 0;             // bytes of the old tail taken
    auto emit = [&](std::vector<Copy>& into, uint8_t dst_space, uint64_t dst, uint64_t want) {
      while (want) {
        if (tailpos < told) {
          const uint64_t c = std::min(want, told - tailpos);
          into.push_back(Copy{kOldTail, dst_space, kBlock * s + tailpos, dst, c});
          tailpos += c, dst += c, want -= c;
          continue;
        }
        const uint64_t j = jobs[seg];
        const uint64_t left = len[j] - segpos;
        if (left == 0) {
          ++seg, segpos = 0;
          continue;
        }
        const uint64_t c = std::min(want, left);
        into.push_back(Copy{kArena, dst_space, off[j] + segpos, dst, c});
        segpos += c, dst += c, want -= c;
      }
    };
    if (nb == 0) {
      emit(P.host_copies, kNewTail, kBlock * slot, r.total);
      P.host_commits.push_back(Commit{s, length[s] - told + r.total, slot, tnew});
      continue;
    }
    uint64_t done = 0;
    while (done < nb) {
      if (cur.blocks == cap) close_piece();
      const uint64_t take = std::min(nb - done, cap - cur.blocks);
      emit(cur.copies, kStaging, cur.bytes, take * kBlock);
      cur.lanes.push_back(Lane{s, cur.bytes, take});
      done += take;
      cur.bytes += take * kBlock;
      cur.blocks += take;
      if (done == nb) {
        emit(cur.copies, kNewTail, kBlock * slot, tnew);
        cur.commits.push_back(Commit{s, length[s] - told + r.total, slot, tnew});
      } else {
        cur.commits.push_back(Commit{s, length[s] - told + done * kBlock, kNoSlot, 0});
      }
    }
  }
  close_piece();
  return P;
}

}  // namespace spack
}  // namespace msha
