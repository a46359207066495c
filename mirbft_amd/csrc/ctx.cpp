// libmirsha: host side of the MI355X batched SHA-256 engine (C ABI in include/mirsha.h).
// This unit owns the context: its creation and destruction, the per-GPU helpers every
// path shares (ctx.hpp), the statistics, policy, status, clock-probe and pinned-memory
// entries, and the ctx_access.hpp functions through which the device entries' units
// (streams.cpp, parts*.cpp, stream_device.cpp, verify.cpp, group.cpp) reach a context.
// The host paths are host_small, host_pipeline and host_direct, entered from
// host_entries.cpp; the raw-pointer batch entries are device_batch.cpp.
#include <hip/hip_runtime.h>

#include <sys/mman.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "ctx.hpp"

using namespace msha;

namespace {

// Reason of the most recent failed context creation in the process
// (msha_last_error(NULL)). A fixed, always NUL-terminated buffer written under a
// mutex: a reader on another thread never sees freed memory. msha_ctx_create_err
// hands the reason back with the call instead (no cross-call state at all).
std::mutex g_create_mu;
char g_create_error[512] = "";

void set_create_error(const std::string& msg, char* errbuf, uint64_t errbuf_len) {
  {
    std::lock_guard<std::mutex> g(g_create_mu);
    std::snprintf(g_create_error, sizeof(g_create_error), "%s", msg.c_str());
  }
  if (errbuf && errbuf_len) std::snprintf(errbuf, (size_t)std::min<uint64_t>(errbuf_len, 1u << 20), "%s", msg.c_str());
}

}  // namespace

namespace msha {

// Split-chaining plan for an n-message launch on d (nullptr: plain launch).
// Consecutive launches use different flag arrays of a ring and unique epochs,
// so a launch never reads another launch's flags.
constexpr uint64_t kSplitRing = 16;
// d's flag ring, zeroed before this returns (msha_ctx_create makes it, while d's
// stream is still empty). Every context counts its epochs from 1 and hipMalloc
// hands back an earlier context's ring as it was left, with that context's
// hand-offs of the same epochs in it, so the zeros must be there before a
// launch's first poll. A hipMemset does not promise that: it may return before
// the fill has run, on the null stream, which the streams here (non-blocking)
// are not ordered with. A segment that found such a flag went ahead of the one
// before it and took the digest slot's old bytes for the chain's state: wrong
// digests for the surplus lanes of the launch, and no error bit.
void ensure_split_flags(Device& d) {
  if (d.split_flags) return;
  const uint64_t bytes = kSplitRing * (uint64_t)d.cus * 2 * sizeof(uint64_t);
  HIPCHK(hipMalloc(&d.split_flags, bytes));
  HIPCHK(hipMemsetAsync(d.split_flags, 0, bytes, d.stream));
  HIPCHK(hipStreamSynchronize(d.stream));
}
const msha::SplitPlan* split_for(Device& d, uint64_t n, int policy, msha::SplitPlan& sp,
                                 int cap) {
  if (!msha::plan_split(n, d.cus, policy, &sp, cap)) return nullptr;
  const uint64_t per = (uint64_t)d.cus * 2;  // plan_split: chains <= SIMDs / 2
  ensure_split_flags(d);
  sp.epoch = ++d.split_epoch;
  sp.flags = d.split_flags + (sp.epoch % kSplitRing) * per;
  return &sp;
}

int fail(msha_ctx* ctx, int code, const std::string& msg) {
  if (ctx) std::snprintf(ctx->err, sizeof(ctx->err), "%s", msg.c_str());
  return code;
}

// Count a kernel launch in the context's counters (atomically: the pageable
// multi-GPU path launches from one thread per GPU) and in the shard's.
void count_launch(msha_ctx* ctx, Device* d, msha::LaunchKind kind) {
  uint64_t* f = nullptr;
  switch (kind) {
    case msha::kLaunchLane: f = &ctx->stats.launches_lane; break;
    case msha::kLaunchPipe: f = &ctx->stats.launches_pipe; break;
    case msha::kLaunchCoop: f = &ctx->stats.launches_coop; break;
    case msha::kLaunchSplit: f = &ctx->stats.launches_split; break;
    case msha::kLaunchDod: f = &ctx->stats.launches_dod; break;
    case msha::kLaunchChain2:
      f = &ctx->stats.launches_coop;
      __atomic_fetch_add(&ctx->stats.launches_chain2, 1, __ATOMIC_RELAXED);
      break;
    case msha::kLaunchChain8:
      f = &ctx->stats.launches_coop;
      __atomic_fetch_add(&ctx->stats.launches_chain8, 1, __ATOMIC_RELAXED);
      break;
    case msha::kLaunchLaneWs:
      f = &ctx->stats.launches_lane;
      __atomic_fetch_add(&ctx->stats.launches_lane_ws, 1, __ATOMIC_RELAXED);
      break;
    default: return;
  }
  __atomic_fetch_add(f, 1, __ATOMIC_RELAXED);
  if (d) d->st.launches++;
}

// Device entry points: the context's first device, its error word zeroed once.
void device_prologue(msha_ctx* ctx, void* stream, hipStream_t* st) {
  if (ctx->devs.empty()) throw MshaError(MSHA_ERR_INVALID_ARG, "context has no device");
  Device& d = ctx->devs[0];
  HIPCHK(hipSetDevice(d.id));
  if (!d.err.p) {  // first device call: a zeroed error word (hipMalloc does not zero)
    d.err.ensure(4);
    HIPCHK(hipMemset(d.err.p, 0, 4));
  }
  *st = stream ? static_cast<hipStream_t>(stream) : d.stream;
}

// Is p inside page-locked host memory the GPU can DMA from (hipHostMalloc /
// hipHostRegister)? Pageable memory makes the query fail; clear that error.
bool is_pinned_host(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

}  // namespace msha

namespace {

// NUMA node of GPU dev: its PCI device's numa_node in sysfs (-1: unknown).
int gpu_numa_node(int dev) {
  char bus[64] = {0};
  if (hipDeviceGetPCIBusId(bus, sizeof bus, dev) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  for (char* c = bus; *c; ++c) *c = (char)std::tolower((unsigned char)*c);
  char path[192];
  std::snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
  FILE* f = std::fopen(path, "r");
  if (!f) return -1;
  int node = -1;
  if (std::fscanf(f, "%d", &node) != 1) node = -1;
  std::fclose(f);
  return node;
}

// Does msha_pinned_alloc stripe its allocations over NUMA nodes? When the
// context's GPUs sit on two or more nodes; MSHA_PINNED_STRIPE=1 forces it (a
// one-node box exercises the path), =0 turns it off.
bool stripe_pinned(const msha_ctx* ctx) {
  if (const char* e = getenv("MSHA_PINNED_STRIPE")) return atoi(e) != 0;
  for (const Device& d : ctx->devs)
    if (d.numa >= 0 && d.numa != ctx->devs[0].numa) return true;
  return false;
}

// A pinned allocation for a multi-socket context: cut into one region per shard,
// in shard order, each preferring its shard's GPU's NUMA node (mbind), touched,
// then page-locked for every GPU (hipHostRegister, portable). A caller that packs
// a batch in message order (the Go adapter) then has each GPU's span -- shards
// are contiguous message ranges -- mostly in its own socket's memory, instead of
// every link reading one socket's. nullptr when a step fails (the caller then
// takes hipHostMalloc); *mapped = the mapping's size.
void* striped_pinned_alloc(const msha_ctx* ctx, uint64_t bytes, uint64_t* mapped) {
  constexpr uint64_t kAlign = 2ull << 20;  // region edges on huge-page boundaries
  const uint64_t size = (std::max<uint64_t>(bytes, 1) + kAlign - 1) & ~(kAlign - 1);
  void* p = mmap(nullptr, size, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (p == MAP_FAILED) return nullptr;
  const uint64_t k = ctx->devs.size();
  for (uint64_t s = 0; s < k; ++s) {
    const int node = ctx->devs[s].numa;
    const uint64_t a = (size / k * s) & ~(kAlign - 1);
    const uint64_t b = s + 1 == k ? size : (size / k * (s + 1)) & ~(kAlign - 1);
    if (node < 0 || node >= 1024 || b <= a) continue;
    unsigned long mask[1024 / (8 * sizeof(unsigned long))] = {0};
    mask[node / (8 * sizeof(unsigned long))] |= 1ul << (node % (8 * sizeof(unsigned long)));
    constexpr int kMpolPreferred = 1;  // <linux/mempolicy.h>; best effort: no error if refused
    (void)syscall(SYS_mbind, static_cast<char*>(p) + a, b - a, kMpolPreferred, mask, 1024ul + 1, 0u);
  }
  // first touch places every page by its region's policy (several threads)
  parallel_ranges(WorkerPool::get(), size / kAlign, size, [&](uint64_t a, uint64_t b) {
    std::memset(static_cast<char*>(p) + a * kAlign, 0, (b - a) * kAlign);
  });
  if (hipHostRegister(p, size, hipHostRegisterPortable) != hipSuccess) {
    (void)hipGetLastError();
    munmap(p, size);
    return nullptr;
  }
  *mapped = size;
  return p;
}

void pinned_release(const std::pair<void*, uint64_t>& a) {
  if (a.second) {
    (void)hipHostUnregister(a.first);
    munmap(a.first, a.second);
  } else {
    (void)hipHostFree(a.first);
  }
}

}  // namespace

extern "C" {

uint32_t msha_abi_version(void) { return MSHA_ABI_VERSION; }

int msha_device_count(int* n) {
  if (!n) return MSHA_ERR_INVALID_ARG;
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) {
    (void)hipGetLastError();
    c = 0;
  }
  *n = c;
  return MSHA_OK;
}

int msha_ctx_create_err(uint32_t device_mask, msha_ctx** out, char* errbuf, uint64_t errbuf_len) {
  if (errbuf && errbuf_len) errbuf[0] = 0;
  if (!out) {
    set_create_error("null out pointer", errbuf, errbuf_len);
    return MSHA_ERR_INVALID_ARG;
  }
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    (void)hipGetLastError();
    set_create_error("no HIP device available (the engine has no CPU fallback)", errbuf, errbuf_len);
    return MSHA_ERR_NO_DEVICE;
  }
  if (device_mask == 0) device_mask = 1;
  msha_ctx* ctx = new (std::nothrow) msha_ctx();
  if (!ctx) {
    set_create_error("host allocation failed", errbuf, errbuf_len);
    return MSHA_ERR_OUT_OF_MEMORY;
  }
  int rc = guarded(ctx, [&] {
    // MSHA_VIRTUAL_SHARDS=k (testing only): a one-device mask is split into k
    // shards on that same GPU, each with its own streams and buffers, so the
    // multi-GPU sharding path can be exercised on a one-GPU box.
    int virt = 1;
    if (const char* e = getenv("MSHA_VIRTUAL_SHARDS")) virt = std::max(1, std::min(8, atoi(e)));
    if ((device_mask & (device_mask - 1)) != 0) virt = 1;
    for (int i = 0; i < 32; ++i) {
      if (!(device_mask & (1u << i))) continue;
      if (i >= count)
        throw MshaError(MSHA_ERR_NO_DEVICE, "device_mask names device " + std::to_string(i) + " but only " +
                                                std::to_string(count) + " visible");
      for (int v = 0; v < virt; ++v) {
        Device d;
        d.id = i;
        HIPCHK(hipSetDevice(i));
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, i));
        d.cus = prop.multiProcessorCount;
        d.numa = gpu_numa_node(i);
        HIPCHK(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&d.copy_stream, hipStreamNonBlocking));
        if (virt == 1) {
          HIPCHK(hipStreamCreateWithFlags(&d.d2h_stream, hipStreamNonBlocking));
          HIPCHK(hipEventCreateWithFlags(&d.ev_k, hipEventDisableTiming));
        }
        HIPCHK(hipEventCreate(&d.ev0));
        HIPCHK(hipEventCreate(&d.ev1));
        HIPCHK(hipEventCreate(&d.ev_up0));
        HIPCHK(hipEventCreate(&d.ev_up1));
        HIPCHK(hipEventCreate(&d.ev_k0));
        HIPCHK(hipEventCreate(&d.ev_p0));
        HIPCHK(hipEventCreate(&d.ev_p1));
        HIPCHK(hipEventCreateWithFlags(&d.ev_meta, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&d.ev_plan, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&d.slot_free[0], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&d.slot_free[1], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&d.chunk_in, hipEventDisableTiming));
        ensure_split_flags(d);
        d.st.device = i;
        d.index = (uint32_t)ctx->devs.size();
        ctx->devs.push_back(std::move(d));
      }
    }
  });
  if (rc != MSHA_OK) {
    set_create_error(std::string(ctx->err), errbuf, errbuf_len);
    for (auto& d : ctx->devs) d.release();
    delete ctx;
    return rc;
  }
  *out = ctx;
  return MSHA_OK;
}

int msha_ctx_create(uint32_t device_mask, msha_ctx** out) {
  return msha_ctx_create_err(device_mask, out, nullptr, 0);
}

void msha_ctx_destroy(msha_ctx* ctx) {
  if (!ctx) return;
  for (auto& d : ctx->devs) {
    (void)hipSetDevice(d.id);
    for (hipStream_t st : {d.stream, d.copy_stream, d.d2h_stream})
      if (st) (void)hipStreamSynchronize(st);
    if (&d == &ctx->devs[0]) {  // their workspaces live on the first device
      ctx->parts_plan.ws.release();
      ctx->parts_route.ws.release();
      ctx->group.ws.release();
    }
    d.release();
  }
  for (const auto& a : ctx->pinned) pinned_release(a);
  delete ctx;
}

const char* msha_last_error(const msha_ctx* ctx) { return ctx ? ctx->err : g_create_error; }

uint64_t msha_last_error_copy(const msha_ctx* ctx, char* buf, uint64_t buf_len) {
  std::unique_lock<std::mutex> lock(ctx ? ctx->mu : g_create_mu);
  const char* e = ctx ? ctx->err : g_create_error;
  const uint64_t n = std::strlen(e);
  if (buf && buf_len) {
    const uint64_t c = std::min(n, buf_len - 1);
    std::memcpy(buf, e, c);
    buf[c] = 0;
  }
  return n;
}

int msha_get_stats(const msha_ctx* ctx, msha_stats* out) {
  if (!ctx || !out) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(ctx->mu);
  *out = ctx->stats;
  return MSHA_OK;
}

int msha_shard_count(const msha_ctx* ctx, uint32_t* n) {
  if (!ctx || !n) return MSHA_ERR_INVALID_ARG;
  *n = (uint32_t)ctx->devs.size();
  return MSHA_OK;
}

int msha_get_shard_stats(const msha_ctx* ctx, uint32_t shard, msha_shard_stats* out) {
  if (!ctx || !out || shard >= ctx->devs.size()) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(ctx->mu);
  *out = ctx->devs[shard].st;
  return MSHA_OK;
}

int msha_set_kernel_policy(msha_ctx* ctx, int policy) {
  if (!ctx) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(ctx->mu);

  if (policy != MSHA_KERNEL_AUTO && policy != MSHA_KERNEL_LANE && policy != MSHA_KERNEL_COOP)
    return fail(ctx, MSHA_ERR_INVALID_ARG, "unknown kernel policy " + std::to_string(policy));
  ctx->kernel_policy = policy;
  return MSHA_OK;
}

int msha_device_status(msha_ctx* ctx) {
  if (!ctx || ctx->devs.empty()) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(ctx->mu);

  uint32_t flag = 0;
  int rc = guarded(ctx, [&] {
    Device& d = ctx->devs[0];
    HIPCHK(hipSetDevice(d.id));
    HIPCHK(hipDeviceSynchronize());
    if (!d.err.p) return;
    HIPCHK(hipMemcpy(&flag, d.err.p, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(d.err.p, 0, 4));
  });
  if (rc != MSHA_OK) return rc;
  // bit 16 (msha_concat_lists_device): alone it is the whole text; with an older bit that
  // bit's code and text stay as they are and this clause follows them
  const char* const concat_text =
      "msha_concat_lists_device: a message was refused (it does not fit d_dst, its d_select entry is >= n_lists, "
      "or its list's part range decreases or spans 2^32 parts or more); its d_msg_off and d_msg_len are zero";
  // bit 32 (msha_dstreams_*): the same rule, after the concat clause when both are raised
  const char* const row_text =
      "msha_dstreams_*: row out of range (a d_row entry >= n); no stream was touched and those digests are zero";
  const std::string concat = ((flag & msha::kErrPartsConcat) ? std::string("; and ") + concat_text : std::string()) +
                             ((flag & msha::kErrStreamRow) ? std::string("; and ") + row_text : std::string());
  if (flag & 2) return fail(ctx, MSHA_ERR_HIP, "split-chain handoff timed out (digests undefined)" + concat);
  if (flag & ~(msha::kErrPartsBegin | msha::kErrPartsList | msha::kErrPartsConcat | msha::kErrStreamRow))
    return fail(ctx, MSHA_ERR_ALIGNMENT, "device arena message start not 16-byte aligned" + concat);
  if (flag & msha::kErrPartsBegin)
    return fail(ctx, MSHA_ERR_INVALID_ARG,
                std::string("msha_hash_actions_device: action_part_begin decreases (begin[i+1] < begin[i]); "
                            "those digests are zero") +
                    ((flag & msha::kErrPartsList) ? "; and action_list out of range (an entry >= n_lists)" : "") +
                    concat);
  if (flag & msha::kErrPartsList)
    return fail(ctx, MSHA_ERR_INVALID_ARG,
                "msha_hash_actions_device_planned: action_list out of range (an entry >= n_lists); "
                "those digests are zero" +
                    concat);
  if (flag & msha::kErrPartsConcat)
    return fail(ctx, MSHA_ERR_INVALID_ARG,
                std::string(concat_text) + ((flag & msha::kErrStreamRow) ? std::string("; and ") + row_text : std::string()));
  if (flag & msha::kErrStreamRow) return fail(ctx, MSHA_ERR_INVALID_ARG, row_text);
  return MSHA_OK;
}

int msha_clock_probe(msha_ctx* ctx, uint32_t blocks_per_lane, msha_clock_info* out) {
  if (!ctx || ctx->devs.empty() || !out || blocks_per_lane == 0 || blocks_per_lane > 100000)
    return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(ctx->mu);

  return guarded(ctx, [&] {
    Device& d = ctx->devs[0];
    HIPCHK(hipSetDevice(d.id));
    const uint32_t wgs = (uint32_t)d.cus * 8;  // 8 waves per SIMD, as the lane kernel runs
    d.probe.ensure(32ull * wgs + 64);
    uint64_t* stamps = d.probe.as<uint64_t>();
    uint32_t* sink = reinterpret_cast<uint32_t*>(stamps + 4ull * wgs);
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    struct Ev {
      hipEvent_t a, b;
      ~Ev() {
        (void)hipEventDestroy(a);
        (void)hipEventDestroy(b);
      }
    } ev{e0, e1};
    HIPCHK(hipEventRecord(e0, d.stream));
    HIPCHK(msha::launch_clock_probe(blocks_per_lane, wgs, stamps, sink, d.stream));
    HIPCHK(hipEventRecord(e1, d.stream));
    HIPCHK(hipStreamSynchronize(d.stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<uint64_t> h(4ull * wgs);
    HIPCHK(hipMemcpy(h.data(), stamps, 8 * h.size(), hipMemcpyDeviceToHost));
    std::vector<double> ghz;
    ghz.reserve(wgs);
    for (uint32_t g = 0; g < wgs; ++g) {
      const uint64_t dt = h[4 * g + 2] - h[4 * g], dr = h[4 * g + 3] - h[4 * g + 1];
      if (dr > 0) ghz.push_back((double)dt / (double)dr * 0.1);  // memrealtime: 100 MHz
    }
    if (ghz.empty()) throw MshaError(MSHA_ERR_HIP, "clock probe: no workgroup advanced memrealtime");
    std::sort(ghz.begin(), ghz.end());
    out->ghz_median = ghz[ghz.size() / 2];
    out->ghz_min = ghz.front();
    out->ghz_max = ghz.back();
    out->kernel_ms = ms;
    out->workgroups = wgs;
    out->blocks_per_lane = blocks_per_lane;
    out->gblocks_per_s = ms > 0 ? (double)wgs * 256 * blocks_per_lane / (ms * 1e-3) / 1e9 : 0;
  });
}

int msha_pinned_alloc(msha_ctx* ctx, uint64_t bytes, void** p) {
  if (!ctx || !p) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(ctx->mu);

  return guarded(ctx, [&] {
    HIPCHK(hipSetDevice(ctx->devs[0].id));
    uint64_t mapped = 0;
    *p = stripe_pinned(ctx) ? striped_pinned_alloc(ctx, bytes, &mapped) : nullptr;
    if (!*p) HIPCHK(hipHostMalloc(p, std::max<uint64_t>(bytes, 1), hipHostMallocPortable));
    ctx->pinned.emplace_back(*p, mapped);
  });
}

int msha_pinned_free(msha_ctx* ctx, void* p) {
  if (!ctx) return MSHA_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(ctx->mu);

  auto it = std::find_if(ctx->pinned.begin(), ctx->pinned.end(), [&](const auto& a) { return a.first == p; });
  if (it == ctx->pinned.end()) return fail(ctx, MSHA_ERR_INVALID_ARG, "pointer not from msha_pinned_alloc");
  const std::pair<void*, uint64_t> a = *it;
  ctx->pinned.erase(it);
  return guarded(ctx, [&] {
    if (a.second) {
      HIPCHK(hipHostUnregister(a.first));
      munmap(a.first, a.second);
    } else {
      HIPCHK(hipHostFree(a.first));
    }
  });
}

}  // extern "C"

// ctx_access.hpp: the context as the translation units beside this one reach it (the
// stream sets, the parts entries, the device stream sets).
namespace msha {

std::mutex& ctx_mutex(const msha_ctx* ctx) { return ctx->mu; }

CtxDevice ctx_first_device(msha_ctx* ctx) {
  hipStream_t st;
  device_prologue(ctx, nullptr, &st);
  const Device& d = ctx->devs[0];
  CtxDevice out;
  out.id = d.id;
  out.cus = d.cus;
  out.stream = st;
  out.err = d.err.as<uint32_t>();
  return out;
}

int ctx_fail(msha_ctx* ctx, int code, const char* msg) { return fail(ctx, code, msg ? msg : ""); }

msha_parts_stats& ctx_parts_stats(msha_ctx* ctx) { return ctx->parts_stats; }

msha_concat_stats& ctx_concat_stats(msha_ctx* ctx) { return ctx->concat_stats; }

msha_verify_stats& ctx_verify_stats(msha_ctx* ctx) { return ctx->verify_stats; }

PartsPlanState& ctx_parts_plan(msha_ctx* ctx) { return ctx->parts_plan; }

PartsRouteState& ctx_parts_route(msha_ctx* ctx) { return ctx->parts_route; }

GroupState& ctx_group_state(msha_ctx* ctx) { return ctx->group; }

msha_group_stats& ctx_group_stats(msha_ctx* ctx) { return ctx->group.stats; }

void ctx_count_launch(msha_ctx* ctx, int kind) { count_launch(ctx, nullptr, static_cast<LaunchKind>(kind)); }

bool ctx_first_device_ready(const msha_ctx* ctx) { return !ctx->devs.empty() && ctx->devs[0].err.p != nullptr; }

}  // namespace msha
