// Device stream sets: the host half of msha_dstreams_* (include/mirsha.h "Device stream
// sets"). A set owns three device arrays on the context's first device, allocated once
// in create; Write, Sum, Snap and Reset are one launch each of stream_device.hip's
// kernels on the caller's stream, with nothing else enqueued and no host wait. The host
// checks what it can see (null pointers, the arena's base alignment, the row count);
// the kernels report the rest through the device error word (msha_device_status).
// Length, export and import are synchronous and move whole streams through a staging
// buffer of their own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/mirsha.h"
#include "ctx_access.hpp"
#include "kernels.hpp"
#include "stream_device.hpp"

struct msha_dstreams {
  msha_ctx* ctx = nullptr;
  msha::CtxDevice dev;
  msha::DstreamRows rows;
  msha_dstreams_stats st{};
};

namespace {

constexpr uint8_t kMagic[4] = {'s', 'h', 'a', 0x03};
constexpr uint64_t kRowBytes = 4 * msha::dstream::kRowDwords;
constexpr uint64_t kMaxRows = 0xFFFFFFFFull;  // n and n_rows stay below it

int hip_fail(msha_ctx* ctx, const char* what, hipError_t e) {
  return msha::ctx_fail(ctx, e == hipErrorOutOfMemory ? MSHA_ERR_OUT_OF_MEMORY : MSHA_ERR_HIP,
                        (std::string(what) + ": " + hipGetErrorString(e)).c_str());
}

inline uint32_t be32(const uint8_t* p) {
  return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
}
inline void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v;
}

struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
  ~EventPair() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

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
}

enum Op { kWrite, kSum, kSnap, kReset };

// One launch on the caller's stream and nothing else. Under MSHA_PARTS_TIMING=1
// (diagnostic, parts.cpp's convention) the launch is timed with HIP events, which makes
// the call wait for the kernel; never on a capturing stream.
template <class Launch>
int device_call(msha_dstreams* s, Op op, uint64_t n_rows, void* stream, const char* what, Launch&& launch) {
  msha_ctx* ctx = s->ctx;
  hipError_t e;
  if ((e = hipSetDevice(s->dev.id)) != hipSuccess) return hip_fail(ctx, "hipSetDevice", e);
  const hipStream_t st = stream ? static_cast<hipStream_t>(stream) : s->dev.stream;
  static const bool timing = msha::env_int("MSHA_PARTS_TIMING", 0) == 1;
  bool timed = false;
  if (timing) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if ((e = hipStreamIsCapturing(st, &cap)) != hipSuccess) return hip_fail(ctx, "hipStreamIsCapturing", e);
    timed = cap == hipStreamCaptureStatusNone;
  }
  EventPair ev;
  if (timed) {
    if ((e = hipEventCreate(&ev.a)) != hipSuccess) return hip_fail(ctx, "hipEventCreate", e);
    if ((e = hipEventCreate(&ev.b)) != hipSuccess) return hip_fail(ctx, "hipEventCreate", e);
    if ((e = hipEventRecord(ev.a, st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
  }
  if ((e = launch(st)) != hipSuccess) return hip_fail(ctx, what, e);
  float ms = 0;
  if (timed) {
    if ((e = hipEventRecord(ev.b, st)) != hipSuccess) return hip_fail(ctx, "hipEventRecord", e);
    if ((e = hipEventSynchronize(ev.b)) != hipSuccess) return hip_fail(ctx, "hipEventSynchronize", e);
    if ((e = hipEventElapsedTime(&ms, ev.a, ev.b)) != hipSuccess) return hip_fail(ctx, "hipEventElapsedTime", e);
  }
  msha_dstreams_stats& t = s->st;
  (op == kWrite ? t.writes : op == kSum ? t.sums : op == kSnap ? t.snaps : t.resets)++;
  t.launches++;
  t.last_rows = n_rows;
  t.last_kernel_ms = ms;
  return MSHA_OK;
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

bool ids_valid(const msha_dstreams* s, const uint64_t* id, uint64_t k) {
  if (!id) return k == s->rows.n;
  for (uint64_t j = 0; j < k; ++j)
    if (id[j] >= s->rows.n) return false;
  return true;
}

// The streams id[j] (id null: all) as packed rows in host memory, after the device has
// finished everything enqueued so far.
int fetch_rows(msha_dstreams* s, const uint64_t* id, uint64_t k, std::vector<uint32_t>* host) {
  msha_ctx* ctx = s->ctx;
  hipError_t e;
  if ((e = hipSetDevice(s->dev.id)) != hipSuccess) return hip_fail(ctx, "hipSetDevice", e);
  if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(ctx, "hipDeviceSynchronize", e);
  host->assign(msha::dstream::kRowDwords * k, 0);
  if (k == 0) return MSHA_OK;
  std::vector<uint32_t> id32;
  if (id) id32.assign(id, id + k);  // checked below n < 2^32
  DeviceBuf ids, packed;
  if (id && (e = hipMalloc(&ids.p, 4 * k)) != hipSuccess) return hip_fail(ctx, "hipMalloc", e);
  if ((e = hipMalloc(&packed.p, kRowBytes * k)) != hipSuccess) return hip_fail(ctx, "hipMalloc", e);
  const hipStream_t q = s->dev.stream;
  if (id && (e = hipMemcpyAsync(ids.p, id32.data(), 4 * k, hipMemcpyHostToDevice, q)) != hipSuccess)
    return hip_fail(ctx, "hipMemcpyAsync", e);
  if ((e = msha::launch_dstream_rows_get(s->rows, static_cast<const uint32_t*>(ids.p), k,
                                         static_cast<uint32_t*>(packed.p), q)) != hipSuccess)
    return hip_fail(ctx, "k_dstream_rows_get launch", e);
  if ((e = hipMemcpyAsync(host->data(), packed.p, kRowBytes * k, hipMemcpyDeviceToHost, q)) != hipSuccess)
    return hip_fail(ctx, "hipMemcpyAsync", e);
  if ((e = hipStreamSynchronize(q)) != hipSuccess) return hip_fail(ctx, "hipStreamSynchronize", e);
  return MSHA_OK;
}

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
  int rc = msha::ctx_first_device(ctx, &s->dev);
  if (rc == MSHA_OK) {
    hipError_t e;
    if ((e = hipMalloc(reinterpret_cast<void**>(&s->rows.state), 32 * n)) != hipSuccess ||
        (e = hipMalloc(reinterpret_cast<void**>(&s->rows.tail), 64 * n)) != hipSuccess ||
        (e = hipMalloc(reinterpret_cast<void**>(&s->rows.length), 8 * n)) != hipSuccess)
      rc = hip_fail(ctx, "hipMalloc", e);
    else if ((e = msha::launch_dstream_reset(s->rows, nullptr, n, s->dev.err, s->dev.stream)) != hipSuccess)
      rc = hip_fail(ctx, "k_dstream_reset launch", e);
    else if ((e = hipStreamSynchronize(s->dev.stream)) != hipSuccess)
      rc = hip_fail(ctx, "hipStreamSynchronize", e);
  }
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
  if (!s) return MSHA_ERR_INVALID_ARG;
  if (n_rows == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  if (!d_arena || !d_part_off || !d_part_len || !d_row_part_begin)
    return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  // the kernel reads aligned 16-byte granules of offsets: they must be granules of addresses
  if (reinterpret_cast<uintptr_t>(d_arena) % MSHA_DEVICE_ALIGN)
    return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "msha_dstreams_write_device: d_arena must be 16-byte aligned");
  const int rc = check_rows(s, "msha_dstreams_write_device", d_row, n_rows);
  if (rc != MSHA_OK) return rc;
  return device_call(s, kWrite, n_rows, stream, "k_dstream_write launch", [&](hipStream_t st) {
    return msha::launch_dstream_write(s->rows, d_arena, d_part_off, d_part_len, d_row_part_begin, d_row, n_rows,
                                      s->dev.err, st);
  });
}

int msha_dstreams_sum_device(msha_dstreams* s, const uint32_t* d_row, uint64_t n_rows, uint8_t* d_out, void* stream) {
  if (!s) return MSHA_ERR_INVALID_ARG;
  if (n_rows == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  if (!d_out) return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  const int rc = check_rows(s, "msha_dstreams_sum_device", d_row, n_rows);
  if (rc != MSHA_OK) return rc;
  return device_call(s, kSum, n_rows, stream, "k_dstream_finish launch", [&](hipStream_t st) {
    return msha::launch_dstream_finish(s->rows, d_row, n_rows, d_out, false, s->dev.err, st);
  });
}

int msha_dstreams_snap_device(msha_dstreams* s, const uint32_t* d_row, uint64_t n_rows, uint8_t* d_out, void* stream) {
  if (!s) return MSHA_ERR_INVALID_ARG;
  if (n_rows == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  if (!d_out) return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  const int rc = check_rows(s, "msha_dstreams_snap_device", d_row, n_rows);
  if (rc != MSHA_OK) return rc;
  return device_call(s, kSnap, n_rows, stream, "k_dstream_finish launch", [&](hipStream_t st) {
    return msha::launch_dstream_finish(s->rows, d_row, n_rows, d_out, true, s->dev.err, st);
  });
}

int msha_dstreams_reset_device(msha_dstreams* s, const uint32_t* d_row, uint64_t n_rows, void* stream) {
  if (!s) return MSHA_ERR_INVALID_ARG;
  if (n_rows == 0) return MSHA_OK;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  const int rc = check_rows(s, "msha_dstreams_reset_device", d_row, n_rows);
  if (rc != MSHA_OK) return rc;
  return device_call(s, kReset, n_rows, stream, "k_dstream_reset launch", [&](hipStream_t st) {
    return msha::launch_dstream_reset(s->rows, d_row, n_rows, s->dev.err, st);
  });
}

int msha_dstreams_length(msha_dstreams* s, const uint64_t* id, uint64_t k, uint64_t* out) {
  if (!s) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  if (!ids_valid(s, id, k))
    return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "msha_dstreams_length: stream id out of range (id NULL: k must be n)");
  if (k && !out) return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  try {
    std::vector<uint32_t> rows;
    const int rc = fetch_rows(s, id, k, &rows);
    if (rc != MSHA_OK) return rc;
    for (uint64_t j = 0; j < k; ++j) {
      const uint32_t* p = &rows[msha::dstream::kRowDwords * j];
      out[j] = (uint64_t)p[25] << 32 | p[24];
    }
  } catch (const std::bad_alloc&) {
    return msha::ctx_fail(s->ctx, MSHA_ERR_OUT_OF_MEMORY, "host allocation failed");
  }
  return MSHA_OK;
}

int msha_dstreams_export(msha_dstreams* s, const uint64_t* id, uint64_t k, uint8_t* out) {
  if (!s) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  if (!ids_valid(s, id, k))
    return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "msha_dstreams_export: stream id out of range (id NULL: k must be n)");
  if (k && !out) return msha::ctx_fail(s->ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  try {
    std::vector<uint32_t> rows;
    const int rc = fetch_rows(s, id, k, &rows);
    if (rc != MSHA_OK) return rc;
    for (uint64_t j = 0; j < k; ++j) {
      const uint32_t* p = &rows[msha::dstream::kRowDwords * j];
      uint8_t* o = out + MSHA_STREAM_STATE_BYTES * j;
      const uint64_t len = (uint64_t)p[25] << 32 | p[24];
      std::memcpy(o, kMagic, 4);
      for (int w = 0; w < 8; ++w) put_be32(o + 4 + 4 * w, p[w]);
      std::memset(o + 36, 0, 64);
      std::memcpy(o + 36, p + 8, len % 64);  // little-endian host, as the GPU
      put_be32(o + 100, (uint32_t)(len >> 32));
      put_be32(o + 104, (uint32_t)len);
    }
  } catch (const std::bad_alloc&) {
    return msha::ctx_fail(s->ctx, MSHA_ERR_OUT_OF_MEMORY, "host allocation failed");
  }
  return MSHA_OK;
}

int msha_dstreams_import(msha_dstreams* s, const uint64_t* id, uint64_t k, const uint8_t* in) {
  if (!s) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  msha_ctx* ctx = s->ctx;
  if (!ids_valid(s, id, k))
    return msha::ctx_fail(ctx, MSHA_ERR_INVALID_ARG, "msha_dstreams_import: stream id out of range (id NULL: k must be n)");
  if (k && !in) return msha::ctx_fail(ctx, MSHA_ERR_INVALID_ARG, "null pointer argument");
  for (uint64_t j = 0; j < k; ++j)
    if (std::memcmp(in + MSHA_STREAM_STATE_BYTES * j, kMagic, 4) != 0)
      return msha::ctx_fail(ctx, MSHA_ERR_INVALID_ARG, "msha_dstreams_import: not an exported SHA-256 state (magic)");
  try {
    // Sequential UnmarshalBinary: of the entries that name one stream the last wins (as
    // msha_streams_import). Only that entry goes to the device: two rows for one stream
    // in one launch would be stored by two lanes in no order.
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
    const uint64_t m = last.size();
    std::vector<uint32_t> id32(m), rows(msha::dstream::kRowDwords * m, 0);
    for (uint64_t j = 0; j < m; ++j) {
      const uint8_t* p = in + MSHA_STREAM_STATE_BYTES * last[j];
      uint32_t* r = &rows[msha::dstream::kRowDwords * j];
      id32[j] = (uint32_t)(id ? id[last[j]] : last[j]);
      for (int w = 0; w < 8; ++w) r[w] = be32(p + 4 + 4 * w);
      const uint64_t len = (uint64_t)be32(p + 100) << 32 | be32(p + 104);
      std::memcpy(r + 8, p + 36, len % 64);  // bytes past length % 64 are stored as zeros
      r[24] = (uint32_t)len;
      r[25] = (uint32_t)(len >> 32);
    }
    hipError_t e;
    if ((e = hipSetDevice(s->dev.id)) != hipSuccess) return hip_fail(ctx, "hipSetDevice", e);
    if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(ctx, "hipDeviceSynchronize", e);
    if (m == 0) return MSHA_OK;
    DeviceBuf ids, packed;
    if ((e = hipMalloc(&ids.p, 4 * m)) != hipSuccess) return hip_fail(ctx, "hipMalloc", e);
    if ((e = hipMalloc(&packed.p, kRowBytes * m)) != hipSuccess) return hip_fail(ctx, "hipMalloc", e);
    const hipStream_t q = s->dev.stream;
    if ((e = hipMemcpyAsync(ids.p, id32.data(), 4 * m, hipMemcpyHostToDevice, q)) != hipSuccess)
      return hip_fail(ctx, "hipMemcpyAsync", e);
    if ((e = hipMemcpyAsync(packed.p, rows.data(), kRowBytes * m, hipMemcpyHostToDevice, q)) != hipSuccess)
      return hip_fail(ctx, "hipMemcpyAsync", e);
    if ((e = msha::launch_dstream_rows_set(s->rows, static_cast<const uint32_t*>(ids.p), m,
                                           static_cast<const uint32_t*>(packed.p), q)) != hipSuccess)
      return hip_fail(ctx, "k_dstream_rows_set launch", e);
    if ((e = hipStreamSynchronize(q)) != hipSuccess) return hip_fail(ctx, "hipStreamSynchronize", e);
  } catch (const std::bad_alloc&) {
    return msha::ctx_fail(ctx, MSHA_ERR_OUT_OF_MEMORY, "host allocation failed");
  }
  return MSHA_OK;
}

int msha_dstreams_get_stats(const msha_dstreams* s, msha_dstreams_stats* out) {
  if (!s || !out) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(msha::ctx_mutex(s->ctx));
  *out = s->st;
  return MSHA_OK;
}

}  // extern "C"
