// Stream sets: resumable batched SHA-256 with hash.Hash semantics (mirsha.h
// "Stream sets"; DESIGN.md "Stream sets"). The host half: per stream the byte count
// and the buffered tail; writes planned by stream_pack.hpp and run piece by piece
// through pinned staging on the resume kernels (stream_kernels.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/mirsha.h"
#include "host_call.hpp"
#include "stream_pack.hpp"
#include "stream_state.hpp"

namespace {

namespace sp = msha::spack;
namespace ss = msha::sstate;

static_assert(ss::kBytes == MSHA_STREAM_STATE_BYTES, "the exported state is MSHA_STREAM_STATE_BYTES long");

// A device buffer and its pinned host twin, grown on demand up to what a piece needs.
struct Staged {
  void* d = nullptr;
  void* h = nullptr;
  uint64_t cap = 0;
  void ensure(uint64_t bytes) {
    if (bytes <= cap) return;
    release();
    const uint64_t want = std::max<uint64_t>(bytes, 4096);
    HIPCHK(hipMalloc(&d, want));
    HIPCHK(hipHostMalloc(&h, want, hipHostMallocPortable));
    cap = want;
  }
  void release() {
    if (d) (void)hipFree(d);
    if (h) (void)hipHostFree(h);
    d = h = nullptr;
    cap = 0;
  }
  template <class T> T* dev(uint64_t byte_off = 0) const { return reinterpret_cast<T*>(static_cast<uint8_t*>(d) + byte_off); }
  template <class T> T* host(uint64_t byte_off = 0) const { return reinterpret_cast<T*>(static_cast<uint8_t*>(h) + byte_off); }
};

inline uint64_t round_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

}  // namespace

struct msha_streams {
  msha_ctx* ctx = nullptr;
  uint64_t n = 0;
  uint64_t staging = 0;     // bytes a piece may stage (a multiple of 64)
  uint64_t piece_lanes = 0; // lanes a piece may hold (staging / 64)
  bool failed = false;
  msha::CtxDevice dev;
  uint32_t* d_state = nullptr;  // n x 8 words
  // stage: a piece's blocks (write) or tails (sum) + the arena slack; meta: per lane
  // [off | work | prefix] (8 bytes each) then [row] (4 bytes), each part 16-byte
  // aligned; out: digests / state rows back
  Staged stage, meta, out;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<uint64_t> length;  // bytes written, per stream
  std::vector<uint8_t> tail;     // 64 bytes a stream; length % 64 of them in use
  std::vector<uint8_t> new_tail; // scratch slots of the write in progress
  msha_streams_stats st{};
};

namespace {

struct MetaLayout {
  uint64_t off, work, prefix, row, bytes;
  explicit MetaLayout(uint64_t lanes) {
    const uint64_t a = round_up(8 * lanes, 16);
    off = 0, work = a, prefix = 2 * a, row = 3 * a;
    bytes = 3 * a + round_up(4 * lanes, 16);
  }
};

// A call on the set: msha::guard() (host_call.hpp) on the set's device. A failure
// leaves the set failed (marks_failed), except a host allocation that failed.
template <class F>
int run(msha_streams* s, bool marks_failed, F&& f) {
  bool host_oom = false;
  const int rc = msha::guard(s->ctx, [&] {
    try {
      HIPCHK(hipSetDevice(s->dev.id));
      f();
    } catch (const std::bad_alloc&) {
      host_oom = true;
      throw;
    }
  });
  if (rc != MSHA_OK && marks_failed && !host_oom) s->failed = true;
  return rc;
}

int failed_set(msha_streams* s) {
  return msha::ctx_fail(s->ctx, MSHA_ERR_HIP, "stream set failed earlier: msha_streams_reset(set, NULL, 0) first");
}

inline uint64_t id_at(const uint64_t* id, uint64_t j) { return id ? id[j] : j; }

// The kernel time of the launch between ev0 and ev1 (both recorded, stream synchronised).
void note_launch(msha_streams* s, int mode, uint64_t lanes) {
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, s->ev0, s->ev1));
  s->st.last_kernel_ms = ms;
  s->st.last_load_mode = (uint32_t)mode;
  s->st.last_lanes = (uint32_t)std::min<uint64_t>(lanes, 0xFFFFFFFFu);
}

// state[id[j]] = vals[8 j ..] (vals null: the IV) for j in [0, k), in pieces of piece_lanes.
void set_rows(msha_streams* s, const uint64_t* id, uint64_t k, const uint32_t* vals) {
  hipStream_t q = s->dev.stream;
  for (uint64_t a = 0; a < k; a += s->piece_lanes) {
    const uint64_t m = std::min(s->piece_lanes, k - a);
    const MetaLayout ml(m);
    s->meta.ensure(ml.bytes);
    uint32_t* row = s->meta.host<uint32_t>(ml.row);
    for (uint64_t j = 0; j < m; ++j) row[j] = (uint32_t)id_at(id, a + j);
    HIPCHK(hipMemcpyAsync(s->meta.dev<uint8_t>(ml.row), row, 4 * m, hipMemcpyHostToDevice, q));
    const uint32_t* dv = nullptr;
    if (vals) {
      s->out.ensure(32 * m);
      std::memcpy(s->out.h, vals + 8 * a, 32 * m);
      HIPCHK(hipMemcpyAsync(s->out.d, s->out.h, 32 * m, hipMemcpyHostToDevice, q));
      dv = s->out.dev<uint32_t>();
    }
    HIPCHK(msha::launch_stream_rows_set(s->d_state, s->meta.dev<uint32_t>(ml.row), dv, m, q));
    HIPCHK(hipStreamSynchronize(q));
  }
}

void release(msha_streams* s) {
  (void)hipSetDevice(s->dev.id);
  if (s->d_state) (void)hipFree(s->d_state);
  s->stage.release();
  s->meta.release();
  s->out.release();
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
}

}  // namespace

extern "C" {

int msha_streams_create(msha_ctx* ctx, uint64_t n, uint64_t staging_bytes, msha_streams** out) {
  if (!ctx || !out) return MSHA_ERR_INVALID_ARG;
  *out = nullptr;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  if (n == 0 || n > 0xFFFFFFFFull) return msha::ctx_fail(ctx, MSHA_ERR_INVALID_ARG, "a stream set holds 1 .. 2^32 - 1 streams");
  msha_streams* s = new (std::nothrow) msha_streams;
  if (!s) return msha::ctx_fail(ctx, MSHA_ERR_OUT_OF_MEMORY, "host allocation failed");
  s->ctx = ctx;
  s->n = n;
  s->staging = sp::staging_bound(staging_bytes);
  s->piece_lanes = s->staging / sp::kBlock;
  const int rc = msha::guard(ctx, [&] {
    s->dev = msha::ctx_first_device(ctx);
    s->length.assign(n, 0);
    s->tail.assign(64 * n, 0);
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&s->d_state), 32 * n));
    HIPCHK(hipEventCreate(&s->ev0));
    HIPCHK(hipEventCreate(&s->ev1));
    set_rows(s, nullptr, n, nullptr);
  });
  if (rc != MSHA_OK) {
    release(s);
    delete s;
    return rc;
  }
  *out = s;
  return MSHA_OK;
}

void msha_streams_destroy(msha_streams* s) {
  if (!s) return;
  {
    std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
    release(s);
  }
  delete s;
}

int msha_streams_write(msha_streams* s, const uint8_t* arena, uint64_t arena_len, const uint64_t* id,
                       const uint64_t* off, const uint64_t* len, uint64_t k) {
  if (!s) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  if (s->failed) return failed_set(s);
  if (k && (!id || !off || !len)) return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  if (!arena && arena_len) return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "null arena");
  if (!sp::valid(s->n, arena_len, id, off, len, k))
    return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "stream id out of range or chunk outside the arena");
  return run(s, true, [&] {
    const sp::Plan P = sp::plan(s->length.data(), id, off, len, k, s->staging);
    s->new_tail.assign(64 * P.slots, 0);
    auto copy = [&](const sp::Copy& c, uint8_t* staging) {
      const uint8_t* src = c.src_space == sp::kArena ? arena + c.src : s->tail.data() + c.src;
      uint8_t* dst = c.dst_space == sp::kStaging ? staging + c.dst : s->new_tail.data() + c.dst;
      std::memcpy(dst, src, c.len);
    };
    auto commit = [&](const sp::Commit& c) {
      s->length[c.id] = c.length;
      if (c.slot != sp::kNoSlot) std::memcpy(&s->tail[64 * c.id], &s->new_tail[64 * c.slot], 64);
    };
    hipStream_t q = s->dev.stream;
    for (const sp::Piece& p : P.pieces) {
      const uint64_t lanes = p.lanes.size();
      const MetaLayout ml(lanes);
      s->stage.ensure(p.bytes + msha::kArenaSlack);
      s->meta.ensure(ml.bytes);
      uint8_t* hs = s->stage.host<uint8_t>();
      for (const sp::Copy& c : p.copies) copy(c, hs);
      uint64_t* ho = s->meta.host<uint64_t>(ml.off);
      uint64_t* hw = s->meta.host<uint64_t>(ml.work);
      uint32_t* hr = s->meta.host<uint32_t>(ml.row);
      for (uint64_t j = 0; j < lanes; ++j) {
        ho[j] = p.lanes[j].off;
        hw[j] = p.lanes[j].nblocks;
        hr[j] = (uint32_t)p.lanes[j].id;
      }
      HIPCHK(hipMemcpyAsync(s->stage.d, hs, p.bytes, hipMemcpyHostToDevice, q));
      HIPCHK(hipMemcpyAsync(s->meta.d, s->meta.h, ml.bytes, hipMemcpyHostToDevice, q));
      int mode = 0;
      HIPCHK(hipEventRecord(s->ev0, q));
      HIPCHK(msha::launch_stream_absorb(s->d_state, s->stage.dev<uint8_t>(), s->meta.dev<uint64_t>(ml.off),
                                      s->meta.dev<uint64_t>(ml.work), s->meta.dev<uint32_t>(ml.row), lanes,
                                      s->dev.err, s->dev.cus, q, &mode));
      HIPCHK(hipEventRecord(s->ev1, q));
      HIPCHK(hipStreamSynchronize(q));
      note_launch(s, mode, lanes);
      s->st.launches_absorb++;
      s->st.pieces++;
      s->st.blocks_absorbed += p.blocks;
      for (const sp::Commit& c : p.commits) commit(c);  // only now: the piece's launch completed
    }
    for (const sp::Copy& c : P.host_copies) copy(c, nullptr);
    for (const sp::Commit& c : P.host_commits) commit(c);
    s->st.writes++;
    s->st.bytes_written += P.bytes;
    if (P.pieces.empty()) s->st.buffered_only_writes++;
  });
}

int msha_streams_sum(msha_streams* s, const uint64_t* id, uint64_t k, uint8_t* out) {
  if (!s) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  if (s->failed) return failed_set(s);
  if (!ss::ids_valid(s->n, id, k)) return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "stream id out of range (id NULL: k must be n)");
  if (k && !out) return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  return run(s, true, [&] {
    hipStream_t q = s->dev.stream;
    for (uint64_t a = 0; a < k; a += s->piece_lanes) {
      const uint64_t m = std::min(s->piece_lanes, k - a);
      const MetaLayout ml(m);
      s->stage.ensure(64 * m + msha::kArenaSlack);
      s->meta.ensure(ml.bytes);
      s->out.ensure(32 * m);
      uint8_t* hs = s->stage.host<uint8_t>();
      uint64_t* ho = s->meta.host<uint64_t>(ml.off);
      uint64_t* hw = s->meta.host<uint64_t>(ml.work);
      uint64_t* hp = s->meta.host<uint64_t>(ml.prefix);
      uint32_t* hr = s->meta.host<uint32_t>(ml.row);
      uint64_t blocks = 0;
      for (uint64_t j = 0; j < m; ++j) {
        const uint64_t r = id_at(id, a + j);
        const uint64_t t = s->length[r] % 64;
        std::memcpy(hs + 64 * j, &s->tail[64 * r], 64);
        ho[j] = 64 * j;
        hw[j] = t;
        hp[j] = s->length[r] - t;
        hr[j] = (uint32_t)r;
        blocks += t < 56 ? 1 : 2;
      }
      HIPCHK(hipMemcpyAsync(s->stage.d, hs, 64 * m, hipMemcpyHostToDevice, q));
      HIPCHK(hipMemcpyAsync(s->meta.d, s->meta.h, ml.bytes, hipMemcpyHostToDevice, q));
      int mode = 0;
      HIPCHK(hipEventRecord(s->ev0, q));
      HIPCHK(msha::launch_stream_finish(s->d_state, s->meta.dev<uint64_t>(ml.prefix), s->stage.dev<uint8_t>(),
                                      s->meta.dev<uint64_t>(ml.off), s->meta.dev<uint64_t>(ml.work),
                                      s->meta.dev<uint32_t>(ml.row), m, s->out.dev<uint8_t>(), s->dev.err,
                                      s->dev.cus, q, &mode));
      HIPCHK(hipEventRecord(s->ev1, q));
      HIPCHK(hipMemcpyAsync(s->out.h, s->out.d, 32 * m, hipMemcpyDeviceToHost, q));
      HIPCHK(hipStreamSynchronize(q));
      note_launch(s, mode, m);
      std::memcpy(out + 32 * a, s->out.h, 32 * m);
      s->st.launches_finish++;
      s->st.blocks_finished += blocks;
    }
    s->st.sums++;
  });
}

int msha_streams_reset(msha_streams* s, const uint64_t* id, uint64_t k) {
  if (!s) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  if (id && s->failed) return failed_set(s);
  if (!id) k = s->n;
  if (!ss::ids_valid(s->n, id, k)) return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "stream id out of range");
  const int rc = run(s, true, [&] {
    set_rows(s, id, k, nullptr);
    for (uint64_t j = 0; j < k; ++j) {
      const uint64_t r = id_at(id, j);
      s->length[r] = 0;
      std::memset(&s->tail[64 * r], 0, 64);
    }
  });
  if (!id && rc == MSHA_OK) s->failed = false;
  return rc;
}

int msha_streams_length(const msha_streams* s, const uint64_t* id, uint64_t k, uint64_t* out) {
  if (!s) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  if (!ss::ids_valid(s->n, id, k) || (k && !out)) return MSHA_ERR_INVALID_ARG;
  for (uint64_t j = 0; j < k; ++j) out[j] = s->length[id_at(id, j)];
  return MSHA_OK;
}

int msha_streams_export(msha_streams* s, const uint64_t* id, uint64_t k, uint8_t* out) {
  if (!s) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  if (s->failed) return failed_set(s);
  if (!ss::ids_valid(s->n, id, k)) return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "stream id out of range (id NULL: k must be n)");
  if (k && !out) return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  return run(s, true, [&] {
    hipStream_t q = s->dev.stream;
    for (uint64_t a = 0; a < k; a += s->piece_lanes) {
      const uint64_t m = std::min(s->piece_lanes, k - a);
      const MetaLayout ml(m);
      s->meta.ensure(ml.bytes);
      s->out.ensure(32 * m);
      uint32_t* hr = s->meta.host<uint32_t>(ml.row);
      for (uint64_t j = 0; j < m; ++j) hr[j] = (uint32_t)id_at(id, a + j);
      HIPCHK(hipMemcpyAsync(s->meta.dev<uint8_t>(ml.row), hr, 4 * m, hipMemcpyHostToDevice, q));
      HIPCHK(msha::launch_stream_rows_get(s->d_state, s->meta.dev<uint32_t>(ml.row), s->out.dev<uint32_t>(), m, q));
      HIPCHK(hipMemcpyAsync(s->out.h, s->out.d, 32 * m, hipMemcpyDeviceToHost, q));
      HIPCHK(hipStreamSynchronize(q));
      const uint32_t* hv = s->out.host<uint32_t>();
      for (uint64_t j = 0; j < m; ++j) {
        const uint64_t r = id_at(id, a + j);
        ss::encode(hv + 8 * j, &s->tail[64 * r], s->length[r], out + ss::kBytes * (a + j));
      }
    }
  });
}

int msha_streams_import(msha_streams* s, const uint64_t* id, uint64_t k, const uint8_t* in) {
  if (!s) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  if (s->failed) return failed_set(s);
  if (!ss::ids_valid(s->n, id, k)) return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "stream id out of range (id NULL: k must be n)");
  if (k && !in) return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  for (uint64_t j = 0; j < k; ++j)
    if (!ss::has_magic(in + ss::kBytes * j))
      return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "not an exported SHA-256 state (magic)");
  return run(s, true, [&] {
    // Of the entries that name one stream the last wins, for state, buffer and length
    // alike. Only that entry goes to the device: two rows for one stream in one
    // k_stream_rows_set launch would be stored by two lanes in no order.
    const std::vector<uint64_t> last = ss::last_wins(id, k);
    const uint64_t m = last.size();
    std::vector<uint64_t> ids(m), lens(m);
    std::vector<uint32_t> vals(8 * m);
    std::vector<uint8_t> bufs(64 * m);
    for (uint64_t j = 0; j < m; ++j) {
      ids[j] = id_at(id, last[j]);
      ss::decode(in + ss::kBytes * last[j], &vals[8 * j], &bufs[64 * j], &lens[j]);
    }
    set_rows(s, m ? ids.data() : nullptr, m, vals.data());
    for (uint64_t j = 0; j < m; ++j) {
      s->length[ids[j]] = lens[j];
      std::memcpy(&s->tail[64 * ids[j]], &bufs[64 * j], 64);
    }
  });
}

int msha_streams_get_stats(const msha_streams* s, msha_streams_stats* out) {
  if (!s || !out) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  *out = s->st;
  return MSHA_OK;
}

int msha_absorb_device(msha_ctx* ctx, uint32_t* d_state, const uint8_t* d_arena, const uint64_t* d_off,
                       const uint64_t* d_nblocks, uint64_t n, void* stream) {
  if (!ctx) return MSHA_ERR_INVALID_ARG;
  if (n == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  if (!d_state || !d_arena || !d_off || !d_nblocks) return msha::ctx_fail(ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  return msha::guard(ctx, [&] {
    msha::CtxDevice d;
    const hipStream_t st = msha::device_entry(ctx, "msha_absorb_device", stream, &d);
    msha::launch_check(msha::launch_stream_absorb(d_state, d_arena, d_off, d_nblocks, nullptr, n, d.err, d.cus, st),
                       "k_stream_absorb launch");
  });
}

int msha_absorb_chain_device(msha_ctx* ctx, uint32_t* d_state, const uint8_t* d_arena, const uint64_t* d_off,
                             const uint64_t* d_nblocks, uint64_t n, void* stream) {
  if (!ctx) return MSHA_ERR_INVALID_ARG;
  if (n == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  if (!d_state || !d_arena || !d_off || !d_nblocks) return msha::ctx_fail(ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  return msha::guard(ctx, [&] {
    msha::CtxDevice d;
    const hipStream_t st = msha::device_entry(ctx, "msha_absorb_chain_device", stream, &d);
    msha::launch_check(msha::launch_absorb_chain8(d_state, d_arena, d_off, d_nblocks, nullptr, n, d.err, st),
                       "k_absorb_chain8 launch");
    msha::ctx_count_launch(ctx, msha::kLaunchChain8);
  });
}

int msha_finish_device(msha_ctx* ctx, const uint32_t* d_state, const uint64_t* d_prefix, const uint8_t* d_arena,
                       const uint64_t* d_off, const uint64_t* d_len, uint64_t n, uint8_t* d_out, void* stream) {
  if (!ctx) return MSHA_ERR_INVALID_ARG;
  if (n == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  if (!d_arena || !d_off || !d_len || !d_out) return msha::ctx_fail(ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  return msha::guard(ctx, [&] {
    msha::CtxDevice d;
    const hipStream_t st = msha::device_entry(ctx, "msha_finish_device", stream, &d);
    msha::launch_check(
        msha::launch_stream_finish(d_state, d_prefix, d_arena, d_off, d_len, nullptr, n, d_out, d.err, d.cus, st),
        "k_stream_finish launch");
  });
}

}  // extern "C"
