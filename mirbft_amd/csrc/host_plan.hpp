// Host planning of libmirsha, HIP-free: the worker pool, the size-class order, the block
// partition, the alias table, the batch scan, the direct path's granule marking and upload
// enumeration, and the latency path's limits. Nothing here makes a HIP call or includes a
// HIP header, so tests/cpp/host_planning_asan.cpp and tools/plan_bench.cpp compile it with
// plain g++ (ASan/UBSan, TSan). Header-only: every function is inline where it is used
// (blocks_for, round16 and the marking and scanning loops are hot per message), and the
// process-wide pool (WorkerPool::get) and the per-thread pool (tl_pool) are one each in
// the library. Used by ctx.hpp, and through it by every host path.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mirsha.h"
#include "msha_error.hpp"

namespace msha {

inline double now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

inline uint64_t blocks_for(uint64_t len) { return (len >> 6) + ((len & 63) < 56 ? 1 : 2); }
inline uint64_t round16(uint64_t x) { return (x + 15) & ~uint64_t(15); }

inline uint64_t env_u64(const char* name, uint64_t dflt) {
  const char* e = getenv(name);
  return e ? strtoull(e, nullptr, 10) : dflt;
}

// Worker pool for those phases (thread creation would otherwise cost ~0.1 ms
// per thread per phase): one process-wide pool, plus one per GPU of a
// multi-GPU context for its gather thread (pageable arenas). run(T, job) calls
// job(t) for t in [0, T) on the workers and the calling thread, and returns
// when all are done. One run at a time: a caller that finds the pool busy
// (another context planning concurrently) runs its tasks on fresh threads.
class WorkerPool {
 public:
  static WorkerPool& get() {
    // 16 threads (one GPU's host share), or MSHA_HOST_THREADS; never above the machine's
    static WorkerPool pool([] {
      const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
      const char* env = getenv("MSHA_HOST_THREADS");
      const unsigned want = env ? (unsigned)std::max(1L, std::strtol(env, nullptr, 10)) : 16u;
      return std::min(want, hw) - 1;
    }());
    return pool;
  }
  explicit WorkerPool(unsigned helpers) {
    for (unsigned i = 0; i < helpers; ++i) workers_.emplace_back([this] { loop(); });
  }
  unsigned size() const { return (unsigned)workers_.size() + 1; }
  void run(unsigned T, const std::function<void(unsigned)>& job) {
    std::unique_lock<std::mutex> busy(run_mu_, std::try_to_lock);
    if (!busy.owns_lock() || workers_.empty()) {
      std::vector<std::thread> th;
      for (unsigned t = 1; t < T; ++t) th.emplace_back(job, t);
      job(0);
      for (auto& x : th) x.join();
      return;
    }
    {
      std::lock_guard<std::mutex> g(mu_);
      job_ = &job;
      ntasks_ = T;
      next_ = 0;
      pending_ = T;
      ++gen_;
    }
    cv_.notify_all();
    work();
    std::unique_lock<std::mutex> g(mu_);
    done_cv_.wait(g, [&] { return pending_ == 0; });
    job_ = nullptr;
  }
  ~WorkerPool() {
    {
      std::lock_guard<std::mutex> g(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& w : workers_) w.join();
  }

 private:
  void work() {  // claim and run tasks of the current generation
    for (;;) {
      unsigned t;
      const std::function<void(unsigned)>* job;
      {
        std::lock_guard<std::mutex> g(mu_);
        if (!job_ || next_ >= ntasks_) return;
        t = next_++;
        job = job_;
      }
      (*job)(t);
      std::lock_guard<std::mutex> g(mu_);
      if (--pending_ == 0) done_cv_.notify_all();
    }
  }
  void loop() {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> g(mu_);
        cv_.wait(g, [&] { return stop_ || gen_ != seen; });
        if (stop_) return;
        seen = gen_;
      }
      work();
    }
  }
  std::vector<std::thread> workers_;
  std::mutex run_mu_, mu_;
  std::condition_variable cv_, done_cv_;
  const std::function<void(unsigned)>* job_ = nullptr;
  unsigned ntasks_ = 0, next_ = 0, pending_ = 0;
  uint64_t gen_ = 0;
  bool stop_ = false;
};

// Host planning of large batches runs on a few threads: [0, n) is split into
// T contiguous chunks and f(t, lo, hi) runs for each (T = 1 below 256 K items).
// The threads are those of the calling thread's pool: the process-wide one,
// or, while one GPU's shard of a multi-GPU call is planned on a thread of its
// own, that GPU's pool (tl_pool), so the shards are planned side by side.
inline thread_local WorkerPool* tl_pool = nullptr;
inline WorkerPool& cur_pool() { return tl_pool ? *tl_pool : WorkerPool::get(); }
inline unsigned plan_threads(uint64_t n) {
  if (n < (1u << 18)) return 1;
  return cur_pool().size();
}
template <class F>
void parallel_chunks(uint64_t n, unsigned T, F&& f) {
  if (T <= 1) {
    f(0u, (uint64_t)0, n);
    return;
  }
  const std::function<void(unsigned)> job = [&](unsigned t) { f(t, n * t / T, n * (t + 1) / T); };
  cur_pool().run(T, job);
}

// Host threads for a call on a context of distinct_gpus physical GPUs: 16 per physical GPU (virtual shards of one
// GPU share its 16), at most the machine's, MSHA_HOST_THREADS overriding. On an
// 8-GPU node each shard then plans its 1/8 of the batch on 16 threads, as one
// GPU plans a whole batch, so planning stays under each link's shorter upload.
inline unsigned host_threads_total(unsigned distinct_gpus) {
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const char* env = getenv("MSHA_HOST_THREADS");
  const unsigned want = env ? (unsigned)std::max(1L, std::strtol(env, nullptr, 10))
                            : 16u * std::max(distinct_gpus, 1u);
  return std::min(want, hw);
}

// The wide pool of a context over several physical GPUs (made on first use, kept in
// `wide`) installed as the calling thread's pool for a scope: guarded() (ctx.hpp).
// distinct_gpus 0 (a context that has no device yet): the caller's pool stays.
struct PoolScope {
  WorkerPool* prev = tl_pool;
  PoolScope(std::unique_ptr<WorkerPool>& wide, unsigned distinct_gpus) {
    if (!distinct_gpus) return;
    const unsigned total = host_threads_total(distinct_gpus);
    if (!wide && total > WorkerPool::get().size()) wide.reset(new WorkerPool(total - 1));
    if (wide) tl_pool = wide.get();
  }
  ~PoolScope() { tl_pool = prev; }
};

// Split [0, n) into nearly equal contiguous pieces and run f(lo, hi) on the
// threads of `pool` (gathering into pinned staging is host-bandwidth bound).
template <class F>
void parallel_ranges(WorkerPool& pool, uint64_t n, uint64_t bytes, F&& f) {
  unsigned t = (unsigned)std::min<uint64_t>({(uint64_t)pool.size(), bytes / (4u << 20) + 1, n});
  if (t <= 1) {
    f(0, n);
    return;
  }
  const std::function<void(unsigned)> job = [&](unsigned k) { f(n * k / t, n * (k + 1) / t); };
  pool.run(t, job);
}

// Descending-block-count permutation so every wavefront gets messages of equal
// length and no lane idles. Stable. Batches rarely hold more than a few dozen
// distinct block counts, so a one-pass counting sort over [0, max blocks]
// (scattered writes into that many sequential streams) is the common path;
// messages beyond 2^20 blocks (64 MiB) fall back to a two-pass LSD radix.
// rep (may be null): only messages with rep[i] == i are ordered (aliases of
// another message get no lane). Returns the number of entries written.
inline uint64_t order_by_blocks_desc(const uint64_t* len, uint64_t n, uint32_t* order,
                              std::vector<uint32_t>& tmp, const uint32_t* rep = nullptr) {
  auto keep = [&](uint64_t i) { return !rep || rep[i] == i; };
  const unsigned T0 = plan_threads(n);
  std::vector<uint64_t> tmax(T0, 0);
  parallel_chunks(n, T0, [&](unsigned t, uint64_t lo, uint64_t hi) {
    uint64_t b = 0;
    for (uint64_t i = lo; i < hi; ++i) b = std::max(b, blocks_for(len[i]));
    tmax[t] = b;
  });
  const uint64_t bmax = *std::max_element(tmax.begin(), tmax.end());
  if (bmax <= (1u << 20)) {
    // per-thread histograms only while all of them together stay small (at most
    // 2^20 counters: a wide pool of 128 threads must not zero and scan 128 x 64 K)
    const uint64_t B = bmax + 1;               // bucket j = block count bmax - j
    const unsigned T = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(T0, (1u << 20) / B));
    std::vector<uint64_t> cnt((uint64_t)T * B, 0);
    parallel_chunks(n, T, [&](unsigned t, uint64_t lo, uint64_t hi) {
      uint64_t* c = cnt.data() + (uint64_t)t * B;
      for (uint64_t i = lo; i < hi; ++i)
        if (keep(i)) c[bmax - blocks_for(len[i])]++;
    });
    uint64_t run = 0;  // stable: bucket-major, then thread (= index) order
    for (uint64_t j = 0; j < B; ++j)
      for (unsigned t = 0; t < T; ++t) {
        const uint64_t c = cnt[(uint64_t)t * B + j];
        cnt[(uint64_t)t * B + j] = run;
        run += c;
      }
    parallel_chunks(n, T, [&](unsigned t, uint64_t lo, uint64_t hi) {
      uint64_t* c = cnt.data() + (uint64_t)t * B;
      for (uint64_t i = lo; i < hi; ++i)
        if (keep(i)) order[c[bmax - blocks_for(len[i])]++] = (uint32_t)i;
    });
    return run;
  }
  uint64_t m = 0;
  for (uint64_t i = 0; i < n; ++i)
    if (keep(i)) order[m++] = (uint32_t)i;
  std::vector<uint32_t> key(n);
  for (uint64_t i = 0; i < n; ++i)
    key[i] = 0xffffffffu - (uint32_t)std::min<uint64_t>(blocks_for(len[i]), 0xffffffffu);
  tmp.resize(m);
  uint32_t* src = order;
  uint32_t* dst = tmp.data();
  for (int shift = 0; shift < 32; shift += 16) {
    std::vector<uint64_t> cnt(65537, 0);
    for (uint64_t q = 0; q < m; ++q) cnt[((key[src[q]] >> shift) & 0xffff) + 1]++;
    for (int d = 0; d < 65536; ++d) cnt[d + 1] += cnt[d];
    for (uint64_t q = 0; q < m; ++q) dst[cnt[(key[src[q]] >> shift) & 0xffff]++] = src[q];
    std::swap(src, dst);
  }
  // two passes: result is back in `order`
  return m;
}

inline bool all_equal_blocks(const uint64_t* len, uint64_t n) {
  if (n == 0) return true;
  uint64_t b0 = blocks_for(len[0]);
  for (uint64_t i = 1; i < n; ++i)
    if (blocks_for(len[i]) != b0) return false;
  return true;
}

// Messages per counted piece of the partition: a bound's scan stays short.
constexpr uint64_t kPiece = 1u << 16;

// csum[p] = blocks of the messages before piece p (P + 1 entries), threaded.
inline void piece_sums(const uint64_t* len, uint64_t n, std::vector<uint64_t>& csum) {
  const uint64_t P = std::max<uint64_t>(1, (n + kPiece - 1) / kPiece);
  csum.assign(P + 1, 0);
  parallel_chunks(P, std::min<unsigned>(plan_threads(n), (unsigned)P), [&](unsigned, uint64_t p0, uint64_t p1) {
    for (uint64_t p = p0; p < p1; ++p) {
      uint64_t sum = 0;
      for (uint64_t i = p * kPiece, e = std::min(n, (p + 1) * kPiece); i < e; ++i) sum += blocks_for(len[i]);
      csum[p + 1] = sum;
    }
  });
  for (uint64_t p = 0; p < P; ++p) csum[p + 1] += csum[p];
}

// bounds[s] = the first message whose block-range midpoint reaches s/k of the
// total: acc_i + b_i / 2 >= total * s / k, in integers 2k acc_i + k b_i >=
// 2 s total (acc_i = blocks before i). Midpoints never decrease, so each bound
// lies in the one piece where the running count crosses the target: one short
// scan per bound over the piece sums (a serial pass over c5's 8 M messages cost
// 30-45 ms before any upload began).
inline void partition_pieces(const uint64_t* len, uint64_t n, uint32_t k, const std::vector<uint64_t>& csum,
                      uint64_t* bounds) {
  const uint64_t P = csum.size() - 1;
  using u128 = unsigned __int128;
  const u128 total = csum[P];
  auto bound = [&](uint32_t s) -> uint64_t {
    const u128 goal = 2 * (u128)s * total;
    // the last piece starting below the target (midpoints of earlier pieces are below it too)
    uint64_t p = 0;
    while (p + 1 < P && (u128)2 * k * csum[p + 1] < goal) ++p;
    const uint64_t a = p * kPiece, b = std::min(n, (p + 1) * kPiece);
    if ((u128)2 * k * csum[p] >= goal) return a;  // the piece's first message already reaches it
    uint64_t acc = csum[p];
    for (uint64_t i = a; i < b; ++i) {
      const uint64_t bi = blocks_for(len[i]);
      if ((u128)2 * k * acc + (u128)k * bi >= goal) return i;
      acc += bi;
    }
    return b;
  };
  bounds[0] = 0;
  for (uint32_t s = 1; s < k; ++s) bounds[s] = bound(s);
  bounds[k] = n;
}

inline void partition(const uint64_t* len, uint64_t n, uint32_t k, uint64_t* bounds) {
  if (k == 1) {
    bounds[0] = 0;
    bounds[1] = n;
    return;
  }
  std::vector<uint64_t> csum;
  piece_sums(len, n, csum);
  partition_pieces(len, n, k, csum, bounds);
}

// Direct-mode uploads go out in device-space pieces of this size, each with its
// own event, so kernels over the lanes whose payloads have landed start while
// the rest is still crossing PCIe (and their digests come back meanwhile).
// (kernels.hpp kDirectChunkShift, which a HIP-free header cannot include: host_direct.cpp asserts they agree)
constexpr uint64_t kDirectChunk = 1ull << 26;

inline uint32_t alias_tag(uint64_t off, uint64_t len) {
  uint64_t h = off ^ (len * 0x9E3779B97F4A7C15ull);  // splitmix64 finalizer over both fields
  h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
  h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((h ^ (h >> 31)) >> 32);
}

// uid[i] = the first index j <= i with (off[j], len[j]) == (off[i], len[i]).
//
// Candidates first: a message whose offset is greater than every earlier
// message's ("forward") cannot repeat an earlier payload, so uid[i] = i. Only
// the others (offset at or below an earlier one) can be aliases. A batch of
// requests and batches packed in order plus a shared pool of EpochChange
// payloads (c5: ~5 % of the actions point back into the pool) has few of them,
// so the table is built over the candidates only and the forward messages just
// probe it (each key has at most one forward message: its offset is unique),
// instead of inserting all n keys (c5, 8 M actions: 22 ms -> a few ms).
// With more than n/4 candidates the table simply takes every message.
//
// The table: open addressing (linear probing) over R regions picked by the key
// hash's top bits. Pass 1 hashes every key and counts keys per (index chunk,
// region); pass 2 scatters (tag << 32 | index) into per-region buckets, in
// index order; pass 3 builds each region's table on its own worker from its
// bucket alone, prefetching the slot of the key kPrefetch ahead (the probes are
// the cost: random accesses into a table far larger than the caches). A table
// entry is (tag << 32) | (index + 1); off/len are dereferenced only on a tag
// match, and "first" is preserved because a region inserts its keys in index order.
inline void alias_uids(const uint64_t* off, const uint64_t* len, uint64_t n, std::vector<uint64_t>& uid,
                std::vector<uint64_t>& table, std::vector<uint64_t>& bucket, std::vector<uint32_t>& tagv) {
  uid.resize(n);
  tagv.resize(n);
  const unsigned T = plan_threads(n);
  // forward messages (uid = self) and the candidate list, in index order
  std::vector<uint64_t> cmax(T, 0);
  parallel_chunks(n, T, [&](unsigned t, uint64_t a, uint64_t b) {
    uint64_t mx = 0;
    for (uint64_t i = a; i < b; ++i) mx = std::max(mx, off[i] + 1);
    cmax[t] = mx;
  });
  // the forward pass also hashes every key (the probe below reads the tags)
  // and copies each candidate's key out while it streams off/len
  struct Cand {
    std::vector<uint32_t> idx;
    std::vector<uint64_t> off, len;
  };
  std::vector<Cand> tcand(T);
  parallel_chunks(n, T, [&](unsigned t, uint64_t a, uint64_t b) {
    uint64_t run = 0;  // max(off + 1) over every earlier message
    for (unsigned u = 0; u < t; ++u) run = std::max(run, cmax[u]);
    Cand& c = tcand[t];
    for (uint64_t i = a; i < b; ++i) {
      tagv[i] = alias_tag(off[i], len[i]);
      if (off[i] + 1 > run) {
        uid[i] = i;
        run = off[i] + 1;
      } else {
        uid[i] = UINT64_MAX;  // candidate: resolved below
        c.idx.push_back((uint32_t)i);
        c.off.push_back(off[i]);
        c.len.push_back(len[i]);
      }
    }
  });
  uint64_t m = 0;
  for (auto& c : tcand) m += c.idx.size();
  if (m == 0) return;
  const bool subset = m <= n / 4;
  // Items of the table: the candidates (subset mode; their keys in compact
  // arrays, so the table build does not miss the cache on every key) or every
  // message. Item k's key is (ko[k], kl[k]); its message is cand[k] (or k).
  std::vector<uint32_t> cand;
  std::vector<uint64_t> cko, ckl;
  if (subset) {
    cand.resize(m);
    cko.resize(m);
    ckl.resize(m);
    std::vector<uint64_t> at(T + 1, 0);
    for (unsigned t = 0; t < T; ++t) at[t + 1] = at[t] + tcand[t].idx.size();
    const std::function<void(unsigned)> copy = [&](unsigned t) {
      const Cand& c = tcand[t];
      std::memcpy(cand.data() + at[t], c.idx.data(), 4 * c.idx.size());
      std::memcpy(cko.data() + at[t], c.off.data(), 8 * c.off.size());
      std::memcpy(ckl.data() + at[t], c.len.data(), 8 * c.len.size());
    };
    if (T == 1) copy(0);
    else WorkerPool::get().run(T, copy);
  } else {
    m = n;
  }
  tcand.clear();
  const uint64_t* ko = subset ? cko.data() : off;
  const uint64_t* kl = subset ? ckl.data() : len;
  bucket.resize(m);
  const unsigned rbits = m >= (1u << 20) ? 4 : 0;
  const unsigned R = 1u << rbits;  // regions (one pass-3 task each)
  const unsigned Tm = plan_threads(m);
  std::vector<uint64_t> cnt((size_t)Tm * R, 0);
  // item k's tag, then (subset mode) the table slot of its key; every
  // message's tag stays in tagv for the forward probe
  std::vector<uint32_t> ctag;
  std::vector<uint32_t>& tag_k = subset ? ctag : tagv;
  if (subset) ctag.resize(m);
  // pass 1: region histogram (subset mode: the candidates' tags, from their keys)
  parallel_chunks(m, Tm, [&](unsigned t, uint64_t a, uint64_t b) {
    uint64_t* c = cnt.data() + (size_t)t * R;
    for (uint64_t k = a; k < b; ++k) {
      const uint32_t tag = subset ? alias_tag(ko[k], kl[k]) : tagv[k];
      tag_k[k] = tag;
      ++c[rbits ? tag >> (32 - rbits) : 0];
    }
  });
  // bucket layout: region-major, chunk order inside a region (= index order)
  std::vector<uint64_t> rstart(R + 1, 0), base((size_t)Tm * R);
  {
    uint64_t acc = 0;
    for (unsigned r = 0; r < R; ++r) {
      rstart[r] = acc;
      for (unsigned t = 0; t < Tm; ++t) {
        base[(size_t)t * R + r] = acc;
        acc += cnt[(size_t)t * R + r];
      }
    }
    rstart[R] = acc;
  }
  // pass 2: scatter
  parallel_chunks(m, Tm, [&](unsigned t, uint64_t a, uint64_t b) {
    uint64_t* w = base.data() + (size_t)t * R;
    for (uint64_t k = a; k < b; ++k) {
      const uint32_t tag = tag_k[k];
      bucket[w[rbits ? tag >> (32 - rbits) : 0]++] = (uint64_t)tag << 32 | k;
    }
  });
  // per-region table capacity: a power of two >= 2x its keys
  std::vector<uint64_t> cap(R), tstart(R + 1, 0);
  for (unsigned r = 0; r < R; ++r) {
    uint64_t c = 16;
    while (c < 2 * (rstart[r + 1] - rstart[r])) c <<= 1;
    cap[r] = c;
    tstart[r + 1] = tstart[r] + c;
  }
  if (table.size() < tstart[R]) table.resize(tstart[R]);
  // pass 3: one task per region. first_k[k] = the first item with k's key;
  // in subset mode tag_k[k] becomes the global slot of k's key (for the
  // forward probe below).
  std::vector<uint32_t> first_k(subset ? m : 0);
  constexpr uint64_t kPrefetch = 16;
  const std::function<void(unsigned)> build = [&](unsigned r) {
    uint64_t* reg = table.data() + tstart[r];
    const uint64_t mask = cap[r] - 1;
    std::memset(reg, 0, cap[r] * sizeof(uint64_t));  // 0 = empty
    const uint64_t* bk = bucket.data() + rstart[r];
    const uint64_t cnt_r = rstart[r + 1] - rstart[r];
    for (uint64_t q = 0; q < cnt_r; ++q) {
      const uint64_t ahead = q + kPrefetch < cnt_r ? bk[q + kPrefetch] : bk[q];
      __builtin_prefetch(reg + ((ahead >> 32) & mask), 1);
      const uint64_t e0 = bk[q];
      const uint64_t k = e0 & 0xffffffffull, tag = e0 & 0xffffffff00000000ull;
      for (uint64_t p = (e0 >> 32) & mask;; p = (p + 1) & mask) {
        const uint64_t e = reg[p];
        uint64_t j = k;
        if (e == 0) {
          reg[p] = tag | (k + 1);
        } else {
          j = (e & 0xffffffffull) - 1;
          if ((e & 0xffffffff00000000ull) != tag || ko[j] != ko[k] || kl[j] != kl[k]) continue;
        }
        if (subset) {
          first_k[k] = (uint32_t)j;
          tag_k[k] = (uint32_t)(tstart[r] + p);
        } else {
          uid[k] = j;
        }
        break;
      }
    }
  };
  if (R == 1) build(0);
  else WorkerPool::get().run(R, build);
  if (!subset) return;
  // Forward messages that carry a candidate's key are its first occurrence
  // (an offset above every earlier one precedes every repeat of it). A 2^20-bit
  // filter over the candidates' tags (128 KiB, cache-resident) turns away
  // almost every forward message before it touches the table.
  std::vector<uint64_t> filter(1u << 14, 0);
  for (uint64_t g = 0; g < tstart[R]; ++g)
    if (table[g]) {
      const uint32_t tag = (uint32_t)(table[g] >> 32);
      filter[(tag >> 6) & 0x3fff] |= 1ull << (tag & 63);
    }
  std::vector<uint64_t> fwd(tstart[R], UINT64_MAX);
  parallel_chunks(n, T, [&](unsigned, uint64_t a, uint64_t b) {
    for (uint64_t i = a; i < b; ++i) {
      if (uid[i] != i) continue;  // candidates: resolved below
      const uint32_t tag = tagv[i];
      if (!((filter[(tag >> 6) & 0x3fff] >> (tag & 63)) & 1)) continue;
      const unsigned r = rbits ? tag >> (32 - rbits) : 0;
      const uint64_t* reg = table.data() + tstart[r];
      const uint64_t mask = cap[r] - 1;
      for (uint64_t p = tag & mask;; p = (p + 1) & mask) {
        const uint64_t e = reg[p];
        if (e == 0) break;
        const uint64_t j = (e & 0xffffffffull) - 1;
        if ((e >> 32) == tag && ko[j] == off[i] && kl[j] == len[i]) {
          fwd[tstart[r] + p] = i;  // i is forward: the first occurrence of the key
          break;
        }
      }
    }
  });
  parallel_chunks(m, Tm, [&](unsigned, uint64_t a, uint64_t b) {
    for (uint64_t k = a; k < b; ++k) {
      const uint64_t f = fwd[tag_k[k]];
      uid[cand[k]] = f != UINT64_MAX ? f : cand[first_k[k]];
    }
  });
}

// The latency path's limits (host_small.hpp).
// Limits, read per call (a getenv is ~0.1 us; tests switch paths within one
// process). Measured per call (tools/latency.cpp, profiles/r02_latency/): packing
// on the calling thread beats the pipeline up to a few MiB (512-B requests: 4,096
// 132 vs 193 us, 16,384 388 vs 448 us; 65,536 = 32 MiB 2.5 vs 1.3 ms); a pinned
// span needs no packing and wins up to one 64 MiB upload piece (65,536 x 512 B 861
// vs 898 us); digest-of-digests keeps its own path above 1 MiB (its table goes up
// once, nothing is gathered: 4,096 Batches 137 us vs 184 packed).
inline uint64_t small_bytes() { return env_u64("MSHA_SMALL_BYTES", 4ull << 20); }   // packed payload; 0 disables
inline uint64_t small_msgs() { return env_u64("MSHA_SMALL_MSGS", 65536); }
inline uint64_t small_span_bytes() { return std::min<uint64_t>(env_u64("MSHA_SMALL_SPAN_BYTES", kDirectChunk), kDirectChunk); }
constexpr uint64_t kSmallSpanMin = 512ull << 10;  // below: pack it anyway (one H2D beats two)
constexpr uint64_t kSmallDodBytes = 1ull << 20;
inline bool small_call(uint64_t n, uint64_t bytes) {
  return n <= small_msgs() && bytes <= small_bytes() && small_bytes() > 0;
}

// Long chains on the direct path: a payload of at least kLongBlocks blocks
// (16 KiB: ~0.8 ms as a chain on the lane kernel, more than an upload piece
// takes to land) when the batch has one; MSHA_HOST_HEAD=0 disables (A/B). A
// context held to the lane kernel (MSHA_KERNEL_LANE) runs no heads, as the
// device-planned path does not: its long payloads stay ordinary lanes.
constexpr uint64_t kLongBlocks = 256;
inline uint64_t long_chain_blocks(uint64_t bmax, uint32_t policy) {
  if (env_u64("MSHA_HOST_HEAD", 1) == 0 || policy == MSHA_KERNEL_LANE) return 0;
  return bmax >= kLongBlocks ? kLongBlocks : 0;
}

// Direct path, pass 1 over one shard's messages (threaded): stage their raw
// (off, len) for the planner kernels (h_off null: the caller's arrays are
// pinned and go up as they are), mark the granules (1 << gs bytes of the
// caller's arena, numbered from glo) their payload bytes touch, and return the
// shard's payload span. Zero-length messages need no bytes and mark nothing
// (so one at the arena's very end uploads nothing past it).
struct ShardSpan {
  uint64_t lo = UINT64_MAX, hi = 0, sum = 0, g0 = UINT64_MAX, g1 = 0;
  // some message starts at or below an earlier message's start (the candidates-
  // first test of alias_uids): only then can two messages share (off, len)
  bool backward = false;
  bool any() const { return hi > 0; }
};

// Granule marks: kMarkTouched (a payload byte is in it), kMarkLong (a payload
// of at least long_blocks blocks is: uploaded first, so the long chains start
// as the call begins, wherever their bytes sit in the caller's arena).
// kMarkCross on granule g: a payload runs on from g into g + 1 -- the two must
// then be uploaded in the same class, or the payload would not be contiguous on
// the device (stage_and_mark closes the long class over such boundaries).
constexpr uint8_t kMarkTouched = 1, kMarkLong = 2, kMarkCross = 4;

template <bool kStage>
ShardSpan stage_and_mark_t(const uint64_t* O, const uint64_t* L, uint64_t m, uint64_t glo, unsigned gs,
                           uint64_t* h_off, uint64_t* h_len, std::vector<uint8_t>& mark, uint64_t long_blocks) {
  const unsigned T = plan_threads(m);
  std::vector<ShardSpan> acc(T);
  std::vector<uint64_t> omin(T, UINT64_MAX), omax(T, 0);
  parallel_chunks(m, T, [&](unsigned t, uint64_t a, uint64_t b) {
    uint64_t lo = UINT64_MAX, hi = 0, sum = 0;
    uint64_t last = UINT64_MAX;  // the granule this thread marked last
    uint64_t first_off = UINT64_MAX, max_off = 0;
    bool backward = false;
    for (uint64_t i = a; i < b; ++i) {
      const uint64_t o = O[i], l = L[i];
      if (kStage) {
        h_off[i] = o;
        h_len[i] = l;
      }
      backward |= i > a && o <= max_off;
      max_off = i > a ? std::max(max_off, o) : o;
      if (i == a) first_off = o;
      if (!l) continue;
      const uint64_t e = o + l;
      lo = std::min(lo, o);
      hi = std::max(hi, e);
      sum += l;
      // consecutive messages mostly share a granule (128 x 512 B per 64 KiB):
      // mark a granule once per run, not once per message
      const uint64_t g0 = (o - glo) >> gs, g1 = (e - 1 - glo) >> gs;
      // Marks only grow, so a granule that already holds the bits needs no
      // atomic: a read first (an EpochChange storm names its few long payloads
      // from every thread -- c5: 419K messages on ~75 granules -- and
      // unconditional read-modify-writes there serialised the marking pass on
      // those cache lines: c5's first kernel 5.0 -> 12.3 ms into the call).
      auto mark_or = [&](uint64_t g, uint8_t bits) {
        if ((__atomic_load_n(&mark[g], __ATOMIC_RELAXED) & bits) != bits)
          __atomic_fetch_or(&mark[g], bits, __ATOMIC_RELAXED);
      };
      if (long_blocks && blocks_for(l) >= long_blocks) {  // threads may race on a granule: atomic OR
        for (uint64_t g = g0; g <= g1; ++g) mark_or(g, kMarkTouched | kMarkLong | (g < g1 ? kMarkCross : 0));
        last = UINT64_MAX;
        continue;
      }
      if (g0 == last && g1 == last) continue;
      for (uint64_t g = g0; g <= g1; ++g) mark_or(g, long_blocks && g < g1 ? kMarkTouched | kMarkCross : kMarkTouched);
      last = g1;
    }
    ShardSpan& r = acc[t];
    r.lo = lo;
    r.hi = hi;
    r.sum = sum;
    r.backward = backward;
    omin[t] = first_off;  // the chunk's first start: compared with the earlier chunks' largest
    omax[t] = max_off;
  });
  ShardSpan sh;
  uint64_t run = 0;
  bool seen = false;
  for (unsigned t = 0; t < T; ++t) {
    const ShardSpan& r = acc[t];
    sh.lo = std::min(sh.lo, r.lo);
    sh.hi = std::max(sh.hi, r.hi);
    sh.sum += r.sum;
    if (omin[t] == UINT64_MAX && omax[t] == 0) continue;  // an empty chunk
    sh.backward |= r.backward || (seen && omin[t] <= run);
    run = seen ? std::max(run, omax[t]) : omax[t];
    seen = true;
  }
  if (sh.any()) {  // the granules of the span's ends are the extreme marked ones
    sh.g0 = (sh.lo - glo) >> gs;
    sh.g1 = (sh.hi - 1 - glo) >> gs;
  }
  if (long_blocks && sh.any()) {
    // A payload crossing from a long granule into a plain one (or back) takes
    // the plain one into the long class: a forward sweep carries the class
    // right across crossed boundaries, a backward sweep left. (A long payload
    // marked every granule it touches, and its boundaries crossed.)
    for (uint64_t g = sh.g0; g < sh.g1; ++g)
      if ((mark[g] & (kMarkLong | kMarkCross)) == (kMarkLong | kMarkCross)) mark[g + 1] |= kMarkLong;
    for (uint64_t g = sh.g1; g-- > sh.g0;)
      if ((mark[g] & kMarkCross) && (mark[g + 1] & kMarkLong)) mark[g] |= kMarkLong;
  }
  return sh;
}

inline ShardSpan stage_and_mark(const uint64_t* O, const uint64_t* L, uint64_t m, uint64_t glo, unsigned gs,
                         uint64_t* h_off, uint64_t* h_len, std::vector<uint8_t>& mark, uint64_t long_blocks) {
  return h_off ? stage_and_mark_t<true>(O, L, m, glo, gs, h_off, h_len, mark, long_blocks)
               : stage_and_mark_t<false>(O, L, m, glo, gs, h_off, h_len, mark, long_blocks);
}

// gmap[g] = device offset of granule gbase + g or UINT64_MAX (not uploaded), g
// < ng; gbase == UINT64_MAX: nothing is marked. Granules holding long payloads
// (kMarkLong) come first, then the other marked ones, each class back to back
// in granule order. Returns the device bytes.
inline uint64_t build_gmap(const std::vector<uint8_t>& mark, uint64_t gbase, uint64_t ng, unsigned gs, uint64_t* gmap) {
  uint64_t dev = 0;
  for (int cls = 0; cls < 2; ++cls)
    for (uint64_t g = 0; g < ng; ++g) {
      const uint8_t mk = gbase != UINT64_MAX ? mark[gbase + g] : 0;
      if (!mk) {
        if (cls == 0) gmap[g] = UINT64_MAX;
        continue;
      }
      if (((mk & kMarkLong) != 0) != (cls == 0)) continue;
      gmap[g] = dev;
      dev += 1ull << gs;
    }
  return dev;
}

// The shard's uploads: f(caller offset, device offset, bytes) for each run of
// mapped granules, clipped to the shard's payload span [lo, hi) (so never past
// the arena), in ascending device order (the long payloads' granules first,
// build_gmap), split where device offsets cross a kDirectChunk boundary.
template <class F>
void for_each_upload(const uint64_t* gmap, const std::vector<uint8_t>& mark, uint64_t ng, uint64_t gbase,
                     uint64_t glo, unsigned gs, uint64_t lo, uint64_t hi, F&& f, uint64_t piece_bytes = kDirectChunk) {
  const uint64_t G = 1ull << gs;
  for (int cls = 0; cls < 2; ++cls) {
    auto in_cls = [&](uint64_t g) {
      return gmap[g] != UINT64_MAX && ((mark[gbase + g] & kMarkLong) != 0) == (cls == 0);
    };
    for (uint64_t g = 0; g < ng;) {
      if (!in_cls(g)) {
        ++g;
        continue;
      }
      uint64_t g1 = g;
      while (g1 < ng && in_cls(g1)) ++g1;  // a run of one class: contiguous on the device
      const uint64_t h0 = std::max(lo, glo + (gbase + g) * G), h1 = std::min(hi, glo + (gbase + g1) * G);
      for (uint64_t pos = h0; pos < h1;) {
        const uint64_t r = pos - glo;
        const uint64_t dev = gmap[(r >> gs) - gbase] + (r & (G - 1));
        const uint64_t piece = std::min(h1 - pos, (dev / piece_bytes + 1) * piece_bytes - dev);
        f(pos, dev, piece);
        pos += piece;
      }
      g = g1;
    }
  }
}

// One pass over a host call's messages (threaded): validation (every message
// inside the arena), the covered span, totals, the OR of the offsets
// (alignment), the largest block count, and the partition's piece sums.
struct BatchScan {
  uint64_t lo = UINT64_MAX, hi = 0, sum = 0, blocks = 0, offbits = 0, bmax = 0;
  std::vector<uint64_t> csum;  // piece_sums() layout
};

inline void scan_batch(const uint8_t* arena, uint64_t arena_len, const uint64_t* off, const uint64_t* len, uint64_t n,
                BatchScan& r) {
  const uint64_t P = std::max<uint64_t>(1, (n + kPiece - 1) / kPiece);
  r.csum.assign(P + 1, 0);
  struct Acc {
    uint64_t lo = UINT64_MAX, hi = 0, sum = 0, offbits = 0, bmax = 0, bad = UINT64_MAX;
  };
  const unsigned T = std::min<unsigned>(plan_threads(n), (unsigned)P);
  std::vector<Acc> acc(T);
  parallel_chunks(P, T, [&](unsigned t, uint64_t p0, uint64_t p1) {
    Acc a;
    for (uint64_t p = p0; p < p1 && a.bad == UINT64_MAX; ++p) {
      // branch-free over the piece (the compiler vectorises it); a piece with a
      // bad message is re-scanned for the first one
      const uint64_t i0 = p * kPiece, i1 = std::min(n, (p + 1) * kPiece);
      uint64_t blocks = 0, lo = a.lo, hi = a.hi, sum = a.sum, bits = a.offbits, bmax = a.bmax, bad = 0;
      for (uint64_t i = i0; i < i1; ++i) {
        const uint64_t o = off[i], l = len[i];
        bad |= (uint64_t)(l > arena_len) | (uint64_t)(o > arena_len - l);
        bits |= o;
        lo = std::min(lo, o);
        hi = std::max(hi, o + l);
        sum += l;
        const uint64_t b = blocks_for(l);
        blocks += b;
        bmax = std::max(bmax, b);
      }
      if (bad) {
        for (uint64_t i = i0; i < i1; ++i)
          if (len[i] > arena_len || off[i] > arena_len - len[i]) {
            a.bad = i;
            break;
          }
        break;
      }
      a.lo = lo;
      a.hi = hi;
      a.sum = sum;
      a.offbits = bits;
      a.bmax = bmax;
      r.csum[p + 1] = blocks;
    }
    acc[t] = a;
  });
  r.offbits = reinterpret_cast<uintptr_t>(arena);
  for (const Acc& a : acc) {  // pieces in index order: the first bad message is reported
    if (a.bad != UINT64_MAX)
      throw MshaError(MSHA_ERR_INVALID_ARG, "message " + std::to_string(a.bad) + " [off+len] outside arena");
    r.lo = std::min(r.lo, a.lo);
    r.hi = std::max(r.hi, a.hi);
    r.sum += a.sum;
    r.offbits |= a.offbits;
    r.bmax = std::max(r.bmax, a.bmax);
  }
  for (uint64_t p = 0; p < P; ++p) r.csum[p + 1] += r.csum[p];
  r.blocks = r.csum[P];
}

// memcpy of a large contiguous range on the calling thread's pool (>= 2 MiB a thread).
inline void copy_threads(uint8_t* dst, const uint8_t* src, uint64_t bytes) {
  WorkerPool& pool = cur_pool();
  const unsigned T = (unsigned)std::min<uint64_t>(pool.size(), std::max<uint64_t>(1, bytes >> 21));
  if (T <= 1) {
    std::memcpy(dst, src, bytes);
    return;
  }
  const std::function<void(unsigned)> job = [&](unsigned t) {
    const uint64_t a = (bytes * t / T) & ~uint64_t(63), b = t + 1 == T ? bytes : (bytes * (t + 1) / T) & ~uint64_t(63);
    std::memcpy(dst + a, src + a, b - a);
  };
  pool.run(T, job);
}

}  // namespace msha
