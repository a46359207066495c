// Device stream sets: the host half of msha_dstreams_* (include/mirsha.h "Device stream
// sets"). A set owns three device arrays on the context's first device, allocated once
// in create; Write, Sum, Snap and Reset are one launch each of stream_device.hip's
// kernels on the caller's stream, with nothing else enqueued and no host wait. The host
// checks what it can see (null pointers, the arena's base alignment, the row count);
// the kernels report the rest through the device error word (msha_device_status).
// Length, export and import are synchronous and move whole streams through a staging
// buffer of their own.
//
// Two device calls are several launches each, with a workspace the set owns.
// msha_dstreams_write_jobs_device: the jobs are grouped by stream on the GPU
// (stream_jobs.hip), then Write's kernel runs over all n streams.
// msha_dstreams_write_routed_device: the rows whose write compresses many blocks are
// found on the GPU, flattened behind their stream's buffered bytes and absorbed by the
// eight-lane chain, the others written as lanes (stream_chain.hip, kernels.hip
// k_absorb_chain8; six launches).
// msha_dstreams_write_jobs_routed_device: the first one's grouping, then the second
// one's six launches over the grouped CSR, which names every stream (no new kernel; the
// workspace of both, stream_jobs_route.hpp). Each workspace is a CallWorkspace and
// follows the workspace rule stated in call_workspace.hpp: it grows only outside stream
// capture, and a call outside capture is ordered after the set's previous call of its
// kind.
#include <hip/hip_runtime.h>

#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/mirsha.h"
#include "call_workspace.hpp"
#include "stream_chain.hpp"
#include "stream_device.hpp"
#include "stream_jobs.hpp"
#include "stream_jobs_route.hpp"
#include "stream_state.hpp"

// The workspace of the jobs calls and what msha_dstreams_jobs_read_order needs of the
// last one.
struct DstreamJobs {
  msha::CallWorkspace ws;
  uint64_t last_jobs = 0;
  uint32_t last_passes = 0;
  msha_dstreams_jobs_stats st{};
};

// The workspace of the routed writes (stream_chain.hpp Layout) and what
// msha_dstreams_route_read needs of the last one.
struct DstreamRoute {
  msha::CallWorkspace ws;
  uint64_t last_slots = 0;
  uint64_t at_row = 0, at_stream = 0, at_claim = 0;  // byte offsets in ws of the last call's arrays
  msha_dstreams_route_stats st{};
};

// The workspace of the routed jobs calls (stream_jobs_route.hpp Layout), its own: a jobs
// call, a routed call and a routed jobs call on one set share no memory. And what
// msha_dstreams_jobs_route_read needs of the last one.
struct DstreamJobsRoute {
  msha::CallWorkspace ws;
  uint64_t last_jobs = 0, last_slots = 0;
  uint64_t at_pairs = 0, at_valid = 0, at_stream = 0, at_claim = 0;  // byte offsets in ws of the last call's arrays
  msha_dstreams_jobs_route_stats st{};
};

struct msha_dstreams {
  msha_ctx* ctx = nullptr;
  msha::CtxDevice dev;
  msha::DstreamRows rows;
  msha_dstreams_stats st{};
  DstreamJobs jobs;
  DstreamRoute route;
  DstreamJobsRoute jobs_route;
};

namespace {

namespace ss = msha::sstate;

static_assert(ss::kBytes == MSHA_STREAM_STATE_BYTES, "the exported state is MSHA_STREAM_STATE_BYTES long");
constexpr uint64_t kRowDwords = msha::dstream::kRowDwords;  // a packed row: state, buffer, length (lo, hi)
constexpr uint64_t kRowBytes = 4 * kRowDwords;
constexpr uint64_t kMaxRows = 0xFFFFFFFFull;  // n and n_rows stay below it

struct DeviceBuf {
  void* p = nullptr;
  ~DeviceBuf() {
    if (p) (void)hipFree(p);
  }
};

void release(msha_dstreams* s) {
  (void)hipSetDevice(s->dev.id);
  if (s->rows.state) (void)hipFree(s->rows.state);
  if (s->rows.tail) (void)hipFree(s->rows.tail);
  if (s->rows.length) (void)hipFree(s->rows.length);
  s->jobs.ws.release();
  s->route.ws.release();
  s->jobs_route.ws.release();
}

// The row arguments every device call shares. Call with the lock held.
int check_rows(msha_dstreams* s, const char* entry, const uint32_t* d_row, uint64_t n_rows) {
  if (n_rows >= kMaxRows)
    return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, (std::string(entry) + ": n_rows must be below 2^32 - 1").c_str());
  if (!d_row && n_rows != s->rows.n)
    return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG,
                          (std::string(entry) + ": d_row NULL names every stream, n_rows must equal n").c_str());
  return MSHA_OK;
}

enum Op { kWrite, kSum, kSnap, kReset };

// The rows checked, then one launch on the caller's stream and nothing else (but what
// MSHA_PARTS_TIMING=1 adds: host_call.hpp LaunchTimer). Call with the lock held.
template <class Launch>
int device_call(msha_dstreams* s, const char* entry, Op op, const uint32_t* d_row, uint64_t n_rows, void* stream,
                const char* what, Launch&& launch) {
  const int rc = check_rows(s, entry, d_row, n_rows);
  if (rc != MSHA_OK) return rc;
  return msha::guard(s->ctx, [&] {
    msha::CtxDevice d;  // the set's own (s->dev): the context's first device
    const hipStream_t st = msha::device_entry(s->ctx, entry, stream, &d);
    msha::LaunchTimer timer(st);
    msha::launch_check(launch(st), what);
    const float ms = timer.stop();
    msha_dstreams_stats& t = s->st;
    (op == kWrite ? t.writes : op == kSum ? t.sums : op == kSnap ? t.snaps : t.resets)++;
    t.launches++;
    t.last_rows = n_rows;
    t.last_kernel_ms = ms;
  });
}

// The streams id[j] (id null: all) as packed rows in host memory, after the device has
// finished everything enqueued so far. Inside guard().
std::vector<uint32_t> fetch_rows(msha_dstreams* s, const uint64_t* id, uint64_t k) {
  HIPCHK(hipSetDevice(s->dev.id));
  HIPCHK(hipDeviceSynchronize());
  std::vector<uint32_t> host(kRowDwords * k, 0);
  if (k == 0) return host;
  std::vector<uint32_t> id32;
  if (id) id32.assign(id, id + k);  // checked below n < 2^32
  DeviceBuf ids, packed;
  if (id) HIPCHK(hipMalloc(&ids.p, 4 * k));
  HIPCHK(hipMalloc(&packed.p, kRowBytes * k));
  const hipStream_t q = s->dev.stream;
  if (id) HIPCHK(hipMemcpyAsync(ids.p, id32.data(), 4 * k, hipMemcpyHostToDevice, q));
  msha::launch_check(msha::launch_dstream_rows_get(s->rows, static_cast<const uint32_t*>(ids.p), k,
                                                   static_cast<uint32_t*>(packed.p), q),
                     "k_dstream_rows_get launch");
  HIPCHK(hipMemcpyAsync(host.data(), packed.p, kRowBytes * k, hipMemcpyDeviceToHost, q));
  HIPCHK(hipStreamSynchronize(q));
  return host;
}

inline uint64_t row_length(const uint32_t* row) { return (uint64_t)row[25] << 32 | row[24]; }

}  // namespace

extern "C" {

int msha_dstreams_create(msha_ctx* ctx, uint64_t n, msha_dstreams** out) {
  if (!ctx || !out) return MSHA_ERR_INVALID_ARG;
  *out = nullptr;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(ctx));
  if (n == 0 || n >= kMaxRows)
    return msha::ctx_fail(ctx, MSHA_ERR_INVALID_ARG, "msha_dstreams_create: a device stream set holds 1 .. 2^32 - 2 streams");
  msha_dstreams* s = new (std::nothrow) msha_dstreams;
  if (!s) return msha::ctx_fail(ctx, MSHA_ERR_OUT_OF_MEMORY, "host allocation failed");
  s->ctx = ctx;
  s->rows.n = n;
  s->jobs.st.tile_jobs = msha::sjobs::kTileJobs;
  const int rc = msha::guard(ctx, [&] {
    s->dev = msha::ctx_first_device(ctx);
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&s->rows.state), 32 * n));
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&s->rows.tail), 64 * n));
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&s->rows.length), 8 * n));
    msha::launch_check(msha::launch_dstream_reset(s->rows, nullptr, n, s->dev.err, s->dev.stream),
                       "k_dstream_reset launch");
    HIPCHK(hipStreamSynchronize(s->dev.stream));
  });
  if (rc != MSHA_OK) {
    release(s);
    delete s;
    return rc;
  }
  *out = s;
  return MSHA_OK;
}

void msha_dstreams_destroy(msha_dstreams* s) {
  if (!s) return;
  {
    std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
    release(s);
  }
  delete s;
}

int msha_dstreams_write_device(msha_dstreams* s, const uint8_t* d_arena, const uint64_t* d_part_off,
                               const uint64_t* d_part_len, const uint64_t* d_row_part_begin, const uint32_t* d_row,
                               uint64_t n_rows, void* stream) {
  static const char* const kEntry = "msha_dstreams_write_device";
  if (!s) return MSHA_ERR_INVALID_ARG;
  if (n_rows == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  if (!d_arena || !d_part_off || !d_part_len || !d_row_part_begin)
    return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  // the kernel reads aligned 16-byte granules of offsets: they must be granules of addresses
  if (reinterpret_cast<uintptr_t>(d_arena) % MSHA_DEVICE_ALIGN)
    return msha::bad_arg(s->ctx, kEntry, "d_arena must be 16-byte aligned");
  return device_call(s, kEntry, kWrite, d_row, n_rows, stream, "k_dstream_write launch", [&](hipStream_t st) {
    return msha::launch_dstream_write(s->rows, d_arena, d_part_off, d_part_len, d_row_part_begin, d_row, n_rows,
                                      s->dev.err, st);
  });
}

int msha_dstreams_write_jobs_device(msha_dstreams* s, const uint8_t* d_arena, const uint32_t* d_job_stream,
                                    const uint64_t* d_job_off, const uint64_t* d_job_len, uint64_t n_jobs,
                                    void* stream) {
  static const char* const kEntry = "msha_dstreams_write_jobs_device";
  namespace sj = msha::sjobs;
  if (!s) return MSHA_ERR_INVALID_ARG;
  if (n_jobs == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  if (!d_arena || !d_job_stream || !d_job_off || !d_job_len)
    return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  if (reinterpret_cast<uintptr_t>(d_arena) % MSHA_DEVICE_ALIGN)
    return msha::bad_arg(s->ctx, kEntry, "d_arena must be 16-byte aligned");
  if (n_jobs >= sj::kMaxJobs) return msha::bad_arg(s->ctx, kEntry, "n_jobs must be below 2^32 - 1");
  const sj::Layout lay(n_jobs, s->rows.n);
  if (!lay.ok) return msha::bad_arg(s->ctx, kEntry, "the workspace size does not fit 64 bits");

  return msha::guard(s->ctx, [&] {
    // a capturing stream allows no allocation: know that before the workspace would grow
    const bool capturing = stream && msha::stream_capturing(static_cast<hipStream_t>(stream));
    DstreamJobs& js = s->jobs;
    js.ws.refuse_growth(kEntry, lay.bytes, capturing);
    msha::CtxDevice d;  // the set's own (s->dev): the context's first device
    const hipStream_t st = msha::device_entry(s->ctx, kEntry, stream, capturing, &d);

    uint8_t* ws = js.ws.acquire(kEntry, lay.bytes, lay.bytes / 4, capturing, st);
    msha::StreamJobsArgs a;
    a.job_stream = d_job_stream;
    a.job_off = d_job_off;
    a.job_len = d_job_len;
    a.n_jobs = n_jobs;
    a.n_streams = s->rows.n;
    a.pairs[0] = reinterpret_cast<uint2*>(ws + lay.pairs[0]);
    a.pairs[1] = reinterpret_cast<uint2*>(ws + lay.pairs[1]);
    a.goff = reinterpret_cast<uint64_t*>(ws + lay.off);
    a.glen = reinterpret_cast<uint64_t*>(ws + lay.len);
    a.counts = reinterpret_cast<uint32_t*>(ws + lay.counts);
    a.begin = reinterpret_cast<uint64_t*>(ws + lay.begin);
    a.err = s->dev.err;
    a.passes = sj::pass_count(s->rows.n);

    msha::LaunchTimer timer(st, !capturing && msha::LaunchTimer::wanted());
    uint32_t sort_launches = 0, row_launches = 0;
    msha::launch_check(msha::launch_stream_jobs(a, st, &sort_launches, &row_launches), "stream jobs launch");
    // Write's kernel over all n streams: a stream without a job stores nothing
    msha::launch_check(msha::launch_dstream_write(s->rows, d_arena, a.goff, a.glen, a.begin, nullptr, s->rows.n,
                                                  s->dev.err, st),
                       "k_dstream_write launch");
    js.last_jobs = n_jobs;
    js.last_passes = a.passes;
    js.ws.commit(st, capturing);
    const float ms = timer.stop();
    msha_dstreams_jobs_stats& t = js.st;
    t.calls++;
    t.jobs += n_jobs;
    t.launches_sort += sort_launches;
    t.launches_rows += row_launches;
    t.launches_write++;
    t.last_passes = a.passes;
    t.last_jobs = n_jobs;
    t.last_kernel_ms = ms;
  });
}

int msha_dstreams_get_jobs_stats(const msha_dstreams* s, msha_dstreams_jobs_stats* out) {
  if (!s || !out) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  *out = s->jobs.st;
  return MSHA_OK;
}

int msha_dstreams_jobs_read_order(msha_dstreams* s, uint32_t* order, uint64_t cap, uint64_t* n_jobs,
                                  uint64_t* n_valid) {
  namespace sj = msha::sjobs;
  if (!s || !n_jobs || !n_valid || (cap && !order)) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  *n_jobs = *n_valid = 0;
  const DstreamJobs& js = s->jobs;
  if (!js.ws.ran()) return MSHA_OK;
  return msha::guard(s->ctx, [&] {
    HIPCHK(hipSetDevice(s->dev.id));
    HIPCHK(hipDeviceSynchronize());
    const sj::Layout lay(js.last_jobs, s->rows.n);
    const uint8_t* ws = js.ws.data();
    uint64_t valid = 0;
    HIPCHK(hipMemcpy(&valid, ws + lay.begin + 8 * s->rows.n, 8, hipMemcpyDeviceToHost));
    *n_jobs = js.last_jobs;
    *n_valid = valid < js.last_jobs ? valid : js.last_jobs;
    const uint64_t k = js.last_jobs < cap ? js.last_jobs : cap;
    if (k == 0) return;
    std::vector<uint32_t> pairs(2 * k);  // (key, job index)
    HIPCHK(hipMemcpy(pairs.data(), ws + lay.pairs[sj::sorted_buffer(js.last_passes)], 8 * k, hipMemcpyDeviceToHost));
    for (uint64_t p = 0; p < k; ++p) order[p] = pairs[2 * p + 1];
  });
}

int msha_dstreams_write_routed_device(msha_dstreams* s, const uint8_t* d_arena, const uint64_t* d_part_off,
                                      const uint64_t* d_part_len, const uint64_t* d_row_part_begin,
                                      const uint32_t* d_row, uint64_t n_rows, const msha_route_opts* opts,
                                      void* stream) {
  static const char* const kEntry = "msha_dstreams_write_routed_device";
  namespace sc = msha::schain;
  if (!s) return MSHA_ERR_INVALID_ARG;
  if (n_rows == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  if (!d_arena || !d_part_off || !d_part_len || !d_row_part_begin)
    return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  if (reinterpret_cast<uintptr_t>(d_arena) % MSHA_DEVICE_ALIGN)
    return msha::bad_arg(s->ctx, kEntry, "d_arena must be 16-byte aligned");
  const int rc = check_rows(s, kEntry, d_row, n_rows);
  if (rc != MSHA_OK) return rc;
  // opts: the long_bytes bounds here, the max_long bound once the device is known
  const int orc = msha::guard(s->ctx, [&] {
    (void)msha::route_opts(kEntry, "row", opts, 0, MSHA_DSTREAMS_ROUTE_LONG_BLOCKS_DEFAULT);
  });
  if (orc != MSHA_OK) return orc;

  return msha::guard(s->ctx, [&] {
    // a capturing stream allows no allocation: know that before the workspace would grow
    const bool capturing = stream && msha::stream_capturing(static_cast<hipStream_t>(stream));
    msha::CtxDevice d;  // the set's own (s->dev): the context's first device
    const hipStream_t st = msha::device_entry(s->ctx, kEntry, stream, capturing, &d);

    const msha_route_opts o = msha::route_opts(kEntry, "row", opts, d.cus, MSHA_DSTREAMS_ROUTE_LONG_BLOCKS_DEFAULT);
    msha::StreamRouteArgs a;
    a.long_blocks = o.long_blocks;
    a.max_long = o.max_long;
    a.long_bytes = o.long_bytes;

    DstreamRoute& rs = s->route;
    const sc::Layout lay(n_rows, a.max_long, a.long_bytes);
    if (!lay.ok) throw msha::MshaError(MSHA_ERR_INVALID_ARG, std::string(kEntry) + ": the workspace size does not fit");
    // the arrays grow with a quarter to spare, the flatten buffer is what was asked for
    uint8_t* ws = rs.ws.acquire(kEntry, lay.bytes, lay.flat / 4, capturing, st);
    a.rows = s->rows;
    a.arena = d_arena;
    a.part_off = d_part_off;
    a.part_len = d_part_len;
    a.begin = d_row_part_begin;
    a.row = d_row;
    a.n_rows = n_rows;
    a.claim = reinterpret_cast<unsigned long long*>(ws + lay.claim);
    a.taken = ws + lay.taken;
    a.slot_row = reinterpret_cast<uint32_t*>(ws + lay.slot_row);
    a.slot_stream = reinterpret_cast<uint32_t*>(ws + lay.slot_stream);
    a.slot_t = reinterpret_cast<uint32_t*>(ws + lay.slot_t);
    a.msg_off = reinterpret_cast<uint64_t*>(ws + lay.msg_off);
    a.msg_len = reinterpret_cast<uint64_t*>(ws + lay.msg_len);
    a.blocks = reinterpret_cast<uint64_t*>(ws + lay.blocks);
    a.flat = ws + lay.flat;
    a.err = s->dev.err;
    a.wave_sum_parts = msha::wave_sum_parts();

    // under MSHA_PARTS_TIMING=1 the claim counters are read back too, which makes the call wait
    msha::LaunchTimer timer(st, !capturing && msha::LaunchTimer::wanted());
    msha::launch_check(msha::launch_sroute_init(a, st), "k_sroute_init launch");
    msha::launch_check(msha::launch_sroute_measure(a, st), "k_sroute_measure launch");
    msha::launch_check(msha::launch_sroute_copy(a, st), "k_sroute_copy launch");
    msha::launch_check(msha::launch_absorb_chain8(s->rows.state, a.flat, a.msg_off, a.blocks, a.slot_stream,
                                                  a.max_long, s->dev.err, st),
                       "k_absorb_chain8 launch");
    msha::ctx_count_launch(s->ctx, msha::kLaunchChain8);
    msha::launch_check(msha::launch_sroute_tail(a, st), "k_sroute_tail launch");
    msha::launch_check(msha::launch_dstream_write_rest(a, st), "k_dstream_write_rest launch");
    rs.last_slots = a.max_long;
    rs.at_row = lay.slot_row;
    rs.at_stream = lay.slot_stream;
    rs.at_claim = lay.claim;
    rs.ws.commit(st, capturing);

    const float ms = timer.stop();
    unsigned long long claim[msha::parts_route::kClaimWords] = {};
    if (timer.enabled()) HIPCHK(hipMemcpy(claim, a.claim, sizeof claim, hipMemcpyDeviceToHost));
    msha_dstreams_route_stats& c = rs.st;
    c.calls++;
    c.rows += n_rows;
    c.launches_route += 2;
    c.launches_copy++;
    c.launches_chain++;
    c.launches_tail++;
    c.launches_write++;
    c.last_routed = claim[msha::parts_route::kClaimRouted];
    c.last_routed_bytes = claim[msha::parts_route::kClaimBytes];
    c.last_kernel_ms = ms;
  });
}

int msha_dstreams_get_route_stats(const msha_dstreams* s, msha_dstreams_route_stats* out) {
  if (!s || !out) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  *out = s->route.st;
  return MSHA_OK;
}

int msha_dstreams_route_read(msha_dstreams* s, uint32_t* rows, uint64_t cap, uint64_t* n_routed,
                             uint64_t* routed_bytes) {
  if (!s || !n_routed || !routed_bytes || (cap && !rows)) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  *n_routed = *routed_bytes = 0;
  const DstreamRoute& rs = s->route;
  if (!rs.ws.ran()) return MSHA_OK;
  return msha::guard(s->ctx, [&] {
    HIPCHK(hipSetDevice(s->dev.id));
    HIPCHK(hipDeviceSynchronize());
    const uint8_t* ws = rs.ws.data();
    const uint64_t m = rs.last_slots;
    std::vector<uint32_t> row(m), strm(m);
    unsigned long long claim[msha::parts_route::kClaimWords] = {};
    HIPCHK(hipMemcpy(row.data(), ws + rs.at_row, 4 * m, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(strm.data(), ws + rs.at_stream, 4 * m, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(claim, ws + rs.at_claim, sizeof claim, hipMemcpyDeviceToHost));
    uint64_t k = 0;
    for (uint64_t j = 0; j < m; ++j) {
      if (strm[j] == msha::schain::kNoStream) continue;  // a slot nobody filled
      if (k < cap) rows[k] = row[j];
      ++k;
    }
    *n_routed = k;
    *routed_bytes = claim[msha::parts_route::kClaimBytes];
  });
}

int msha_dstreams_write_jobs_routed_device(msha_dstreams* s, const uint8_t* d_arena, const uint32_t* d_job_stream,
                                           const uint64_t* d_job_off, const uint64_t* d_job_len, uint64_t n_jobs,
                                           const msha_route_opts* opts, void* stream) {
  static const char* const kEntry = "msha_dstreams_write_jobs_routed_device";
  namespace sj = msha::sjobs;
  if (!s) return MSHA_ERR_INVALID_ARG;
  if (n_jobs == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  if (!d_arena || !d_job_stream || !d_job_off || !d_job_len)
    return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  if (reinterpret_cast<uintptr_t>(d_arena) % MSHA_DEVICE_ALIGN)
    return msha::bad_arg(s->ctx, kEntry, "d_arena must be 16-byte aligned");
  if (n_jobs >= sj::kMaxJobs) return msha::bad_arg(s->ctx, kEntry, "n_jobs must be below 2^32 - 1");
  // opts: the long_bytes bounds here, the max_long bound once the device is known
  const int orc = msha::guard(s->ctx, [&] {
    (void)msha::route_opts(kEntry, "stream", opts, 0, MSHA_DSTREAMS_ROUTE_LONG_BLOCKS_DEFAULT);
  });
  if (orc != MSHA_OK) return orc;

  return msha::guard(s->ctx, [&] {
    // a capturing stream allows no allocation: know that before the workspace would grow
    const bool capturing = stream && msha::stream_capturing(static_cast<hipStream_t>(stream));
    msha::CtxDevice d;  // the set's own (s->dev): the context's first device
    const hipStream_t st = msha::device_entry(s->ctx, kEntry, stream, capturing, &d);

    const msha_route_opts o = msha::route_opts(kEntry, "stream", opts, d.cus, MSHA_DSTREAMS_ROUTE_LONG_BLOCKS_DEFAULT);
    const uint64_t n = s->rows.n;
    DstreamJobsRoute& jr = s->jobs_route;
    const msha::sjroute::Layout lay(n_jobs, n, o.max_long, o.long_bytes);
    if (!lay.ok) throw msha::MshaError(MSHA_ERR_INVALID_ARG, std::string(kEntry) + ": the workspace size does not fit");
    // the arrays grow with a quarter to spare, the flatten buffer is what was asked for
    uint8_t* ws = jr.ws.acquire(kEntry, lay.bytes, lay.arrays / 4, capturing, st);

    msha::StreamJobsArgs j;
    j.job_stream = d_job_stream;
    j.job_off = d_job_off;
    j.job_len = d_job_len;
    j.n_jobs = n_jobs;
    j.n_streams = n;
    j.pairs[0] = reinterpret_cast<uint2*>(ws + lay.jobs.pairs[0]);
    j.pairs[1] = reinterpret_cast<uint2*>(ws + lay.jobs.pairs[1]);
    j.goff = reinterpret_cast<uint64_t*>(ws + lay.jobs.off);
    j.glen = reinterpret_cast<uint64_t*>(ws + lay.jobs.len);
    j.counts = reinterpret_cast<uint32_t*>(ws + lay.jobs.counts);
    j.begin = reinterpret_cast<uint64_t*>(ws + lay.jobs.begin);
    j.err = s->dev.err;
    j.passes = sj::pass_count(n);

    // the routed write over the grouped CSR: row r is stream r, every stream a row, a
    // stream without a valid job a row without parts; the dropped jobs lie behind begin[n]
    msha::StreamRouteArgs a;
    a.long_blocks = o.long_blocks;
    a.max_long = o.max_long;
    a.long_bytes = o.long_bytes;
    a.rows = s->rows;
    a.arena = d_arena;
    a.part_off = j.goff;
    a.part_len = j.glen;
    a.begin = j.begin;
    a.row = nullptr;
    a.n_rows = n;
    a.claim = reinterpret_cast<unsigned long long*>(ws + lay.claim);
    a.taken = ws + lay.taken;
    a.slot_row = reinterpret_cast<uint32_t*>(ws + lay.slot_row);
    a.slot_stream = reinterpret_cast<uint32_t*>(ws + lay.slot_stream);
    a.slot_t = reinterpret_cast<uint32_t*>(ws + lay.slot_t);
    a.msg_off = reinterpret_cast<uint64_t*>(ws + lay.msg_off);
    a.msg_len = reinterpret_cast<uint64_t*>(ws + lay.msg_len);
    a.blocks = reinterpret_cast<uint64_t*>(ws + lay.blocks);
    a.flat = ws + lay.flat;
    a.err = s->dev.err;
    a.wave_sum_parts = msha::wave_sum_parts();

    // under MSHA_PARTS_TIMING=1 the claim counters are read back too, which makes the call wait
    msha::LaunchTimer timer(st, !capturing && msha::LaunchTimer::wanted());
    uint32_t sort_launches = 0, row_launches = 0;
    msha::launch_check(msha::launch_stream_jobs(j, st, &sort_launches, &row_launches), "stream jobs launch");
    msha::launch_check(msha::launch_sroute_init(a, st), "k_sroute_init launch");
    msha::launch_check(msha::launch_sroute_measure(a, st), "k_sroute_measure launch");
    msha::launch_check(msha::launch_sroute_copy(a, st), "k_sroute_copy launch");
    msha::launch_check(msha::launch_absorb_chain8(s->rows.state, a.flat, a.msg_off, a.blocks, a.slot_stream,
                                                  a.max_long, s->dev.err, st),
                       "k_absorb_chain8 launch");
    msha::ctx_count_launch(s->ctx, msha::kLaunchChain8);
    msha::launch_check(msha::launch_sroute_tail(a, st), "k_sroute_tail launch");
    msha::launch_check(msha::launch_dstream_write_rest(a, st), "k_dstream_write_rest launch");
    jr.last_jobs = n_jobs;
    jr.last_slots = a.max_long;
    jr.at_pairs = lay.jobs.pairs[sj::sorted_buffer(j.passes)];
    jr.at_valid = lay.jobs.begin + 8 * n;
    jr.at_stream = lay.slot_stream;
    jr.at_claim = lay.claim;
    jr.ws.commit(st, capturing);

    const float ms = timer.stop();
    unsigned long long claim[msha::parts_route::kClaimWords] = {};
    if (timer.enabled()) HIPCHK(hipMemcpy(claim, a.claim, sizeof claim, hipMemcpyDeviceToHost));
    msha_dstreams_jobs_route_stats& c = jr.st;
    c.calls++;
    c.jobs += n_jobs;
    c.launches_sort += sort_launches;
    c.launches_rows += row_launches;
    c.launches_route += 2;
    c.launches_copy++;
    c.launches_chain++;
    c.launches_tail++;
    c.launches_write++;
    c.last_passes = j.passes;
    c.last_jobs = n_jobs;
    c.last_routed = claim[msha::parts_route::kClaimRouted];
    c.last_routed_bytes = claim[msha::parts_route::kClaimBytes];
    c.last_kernel_ms = ms;
  });
}

int msha_dstreams_get_jobs_route_stats(const msha_dstreams* s, msha_dstreams_jobs_route_stats* out) {
  if (!s || !out) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  *out = s->jobs_route.st;
  return MSHA_OK;
}

int msha_dstreams_jobs_route_read(msha_dstreams* s, uint32_t* order, uint64_t order_cap, uint64_t* n_jobs,
                                  uint64_t* n_valid, uint32_t* streams, uint64_t streams_cap, uint64_t* n_routed,
                                  uint64_t* routed_bytes) {
  if (!s || !n_jobs || !n_valid || !n_routed || !routed_bytes || (order_cap && !order) || (streams_cap && !streams))
    return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  *n_jobs = *n_valid = *n_routed = *routed_bytes = 0;
  const DstreamJobsRoute& jr = s->jobs_route;
  if (!jr.ws.ran()) return MSHA_OK;
  return msha::guard(s->ctx, [&] {
    HIPCHK(hipSetDevice(s->dev.id));
    HIPCHK(hipDeviceSynchronize());
    const uint8_t* ws = jr.ws.data();
    uint64_t valid = 0;
    HIPCHK(hipMemcpy(&valid, ws + jr.at_valid, 8, hipMemcpyDeviceToHost));
    *n_jobs = jr.last_jobs;
    *n_valid = valid < jr.last_jobs ? valid : jr.last_jobs;
    const uint64_t k = jr.last_jobs < order_cap ? jr.last_jobs : order_cap;
    if (k) {
      std::vector<uint32_t> pairs(2 * k);  // (key, job index)
      HIPCHK(hipMemcpy(pairs.data(), ws + jr.at_pairs, 8 * k, hipMemcpyDeviceToHost));
      for (uint64_t p = 0; p < k; ++p) order[p] = pairs[2 * p + 1];
    }
    const uint64_t m = jr.last_slots;
    std::vector<uint32_t> strm(m);
    unsigned long long claim[msha::parts_route::kClaimWords] = {};
    if (m) HIPCHK(hipMemcpy(strm.data(), ws + jr.at_stream, 4 * m, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(claim, ws + jr.at_claim, sizeof claim, hipMemcpyDeviceToHost));
    uint64_t r = 0;
    for (uint64_t i = 0; i < m; ++i) {
      if (strm[i] == msha::schain::kNoStream) continue;  // a slot nobody filled
      if (r < streams_cap) streams[r] = strm[i];
      ++r;
    }
    *n_routed = r;
    *routed_bytes = claim[msha::parts_route::kClaimBytes];
  });
}

int msha_dstreams_sum_device(msha_dstreams* s, const uint32_t* d_row, uint64_t n_rows, uint8_t* d_out, void* stream) {
  if (!s) return MSHA_ERR_INVALID_ARG;
  if (n_rows == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  if (!d_out) return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  return device_call(s, "msha_dstreams_sum_device", kSum, d_row, n_rows, stream, "k_dstream_finish launch",
                     [&](hipStream_t st) {
    return msha::launch_dstream_finish(s->rows, d_row, n_rows, d_out, false, s->dev.err, st);
  });
}

int msha_dstreams_snap_device(msha_dstreams* s, const uint32_t* d_row, uint64_t n_rows, uint8_t* d_out, void* stream) {
  if (!s) return MSHA_ERR_INVALID_ARG;
  if (n_rows == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  if (!d_out) return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  return device_call(s, "msha_dstreams_snap_device", kSnap, d_row, n_rows, stream, "k_dstream_finish launch",
                     [&](hipStream_t st) {
    return msha::launch_dstream_finish(s->rows, d_row, n_rows, d_out, true, s->dev.err, st);
  });
}

int msha_dstreams_reset_device(msha_dstreams* s, const uint32_t* d_row, uint64_t n_rows, void* stream) {
  if (!s) return MSHA_ERR_INVALID_ARG;
  if (n_rows == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  return device_call(s, "msha_dstreams_reset_device", kReset, d_row, n_rows, stream, "k_dstream_reset launch",
                     [&](hipStream_t st) {
    return msha::launch_dstream_reset(s->rows, d_row, n_rows, s->dev.err, st);
  });
}

int msha_dstreams_length(msha_dstreams* s, const uint64_t* id, uint64_t k, uint64_t* out) {
  if (!s) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  if (!ss::ids_valid(s->rows.n, id, k))
    return msha::bad_arg(s->ctx, "msha_dstreams_length", "stream id out of range (id NULL: k must be n)");
  if (k && !out) return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  return msha::guard(s->ctx, [&] {
    const std::vector<uint32_t> rows = fetch_rows(s, id, k);
    for (uint64_t j = 0; j < k; ++j) out[j] = row_length(&rows[kRowDwords * j]);
  });
}

int msha_dstreams_export(msha_dstreams* s, const uint64_t* id, uint64_t k, uint8_t* out) {
  if (!s) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  if (!ss::ids_valid(s->rows.n, id, k))
    return msha::bad_arg(s->ctx, "msha_dstreams_export", "stream id out of range (id NULL: k must be n)");
  if (k && !out) return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  return msha::guard(s->ctx, [&] {
    const std::vector<uint32_t> rows = fetch_rows(s, id, k);
    for (uint64_t j = 0; j < k; ++j) {
      const uint32_t* p = &rows[kRowDwords * j];
      // the buffer's bytes as they lie in the row: little-endian host, as the GPU
      ss::encode(p, reinterpret_cast<const uint8_t*>(p + 8), row_length(p), out + ss::kBytes * j);
    }
  });
}

int msha_dstreams_import(msha_dstreams* s, const uint64_t* id, uint64_t k, const uint8_t* in) {
  if (!s) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  if (!ss::ids_valid(s->rows.n, id, k))
    return msha::bad_arg(s->ctx, "msha_dstreams_import", "stream id out of range (id NULL: k must be n)");
  if (k && !in) return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  for (uint64_t j = 0; j < k; ++j)
    if (!ss::has_magic(in + ss::kBytes * j))
      return msha::bad_arg(s->ctx, "msha_dstreams_import", "not an exported SHA-256 state (magic)");
  return msha::guard(s->ctx, [&] {
    // Only the entry that takes effect goes to the device: two rows for one stream in one
    // launch would be stored by two lanes in no order.
    const std::vector<uint64_t> last = ss::last_wins(id, k);
    const uint64_t m = last.size();
    std::vector<uint32_t> id32(m), rows(kRowDwords * m, 0);
    for (uint64_t j = 0; j < m; ++j) {
      uint32_t* r = &rows[kRowDwords * j];
      uint64_t len = 0;
      id32[j] = (uint32_t)(id ? id[last[j]] : last[j]);
      ss::decode(in + ss::kBytes * last[j], r, reinterpret_cast<uint8_t*>(r + 8), &len);
      r[24] = (uint32_t)len;
      r[25] = (uint32_t)(len >> 32);
    }
    HIPCHK(hipSetDevice(s->dev.id));
    HIPCHK(hipDeviceSynchronize());
    if (m == 0) return;
    DeviceBuf ids, packed;
    HIPCHK(hipMalloc(&ids.p, 4 * m));
    HIPCHK(hipMalloc(&packed.p, kRowBytes * m));
    const hipStream_t q = s->dev.stream;
    HIPCHK(hipMemcpyAsync(ids.p, id32.data(), 4 * m, hipMemcpyHostToDevice, q));
    HIPCHK(hipMemcpyAsync(packed.p, rows.data(), kRowBytes * m, hipMemcpyHostToDevice, q));
    msha::launch_check(msha::launch_dstream_rows_set(s->rows, static_cast<const uint32_t*>(ids.p), m,
                                                     static_cast<const uint32_t*>(packed.p), q),
                       "k_dstream_rows_set launch");
    HIPCHK(hipStreamSynchronize(q));
  });
}

int msha_dstreams_get_stats(const msha_dstreams* s, msha_dstreams_stats* out) {
  if (!s || !out) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  *out = s->st;
  return MSHA_OK;
}

}  // extern "C"
