/*
 * mirsha.h -- C ABI of the MI355X batched SHA-256 digest engine for MirBFT's
 * hash path (libmirsha.so, built from mirbft_amd/csrc/).
 *
 * This is the drop-in boundary. In the reference, hashing is
 *
 *   processor.Hasher                 /root/reference/pkg/processor/serial.go:21-23
 *       New() hash.Hash              (crypto.SHA256: mirbft_test.go:392, testengine/recorder.go:781)
 *   processor.ProcessHashActions     /root/reference/pkg/processor/serial.go:180-198
 *       (hasher, *ActionList) -> (*EventList, error)
 *
 * called once per accumulated ActionList from Node.doHashWork
 * (/root/reference/mirbft.go:282-302) and from the testengine
 * (/root/reference/pkg/testengine/recorder.go:604-610). A cgo adapter packs the
 * ActionList's [][]byte parts into one arena (cgo forbids passing Go memory that
 * holds Go pointers, so [][]byte cannot cross as-is) and makes ONE call below per
 * list; see INTEGRATION.md for the binding.
 *
 * Conventions
 *  - Every function returns MSHA_OK (0) or a positive MSHA_ERR_* code; nothing
 *    throws or aborts across the ABI. msha_last_error() describes the last
 *    failure on a context (or, for ctx == NULL, the last failed context
 *    creation in the process; msha_ctx_create_err returns it with the call).
 *  - Host pointers are owned by the caller and only used during the call; the
 *    library copies into its own pinned staging and device memory and never
 *    retains them. Digests are written to caller memory (32 bytes each, in input
 *    order), so the caller can hand out fresh copies (the state machine keeps
 *    digests as map keys: batch_tracker.go:85-91, epoch_change.go:42-50).
 *  - A context may be shared between threads: calls on one context are
 *    serialised inside the library (a second caller waits for the first; the
 *    reference hashes on one goroutine anyway, mirbft.go:470), and distinct
 *    contexts run concurrently. msha_last_error(ctx) is the context's last
 *    failure, whichever thread made it. Each call selects its device(s)
 *    explicitly, so OS-thread migration between calls (goroutines) is harmless.
 *  - There is no CPU fallback: with no usable GPU, msha_ctx_create fails with
 *    MSHA_ERR_NO_DEVICE.
 */
#ifndef MIRSHA_H_
#define MIRSHA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSHA_ABI_VERSION 10u

enum {
  MSHA_OK = 0,
  MSHA_ERR_INVALID_ARG = 1, /* null pointer, range outside arena, bad bounds */
  MSHA_ERR_NO_DEVICE = 2,   /* no GPU, or device_mask names a missing device */
  MSHA_ERR_HIP = 3,         /* a HIP runtime call failed (message has details) */
  MSHA_ERR_OUT_OF_MEMORY = 4,
  MSHA_ERR_ALIGNMENT = 5    /* device-resident message not 16-byte aligned */
};

/* Bytes that must stay readable after the last message of a DEVICE arena
 * passed to the *_device entry points (the kernels read a message's final
 * block as one whole 64-byte block; bytes past each message are masked). */
#define MSHA_DEVICE_ARENA_SLACK 64u
/* Device-resident message starts must be multiples of this. */
#define MSHA_DEVICE_ALIGN 16u

typedef struct msha_ctx msha_ctx;

typedef struct {
  uint64_t calls;          /* batch calls completed */
  uint64_t messages;       /* digests produced */
  uint64_t message_bytes;  /* sum of unpadded message lengths */
  uint64_t blocks;         /* 64-byte compressions performed */
  /* Last host-memory call, milliseconds of wall time: */
  double plan_ms;          /* host planning: validation .. every shard's work queued (pinned
                              arenas: .. the last shard's kernels queued, lanes planned on the GPU) */
  double pack_ms;          /* gathering payload bytes into pinned staging (summed over shards) */
  double device_ms;        /* first upload .. last kernel on the device (HIP events, max over GPUs;
                              msha_shard_stats splits it into upload_ms and kernel_ms) */
  double total_ms;         /* whole call */
  uint64_t direct_calls;   /* host calls whose arena was uploaded as is (pinned, 16-B aligned) */
  /* Kernel launches by kind, cumulative over every entry point: */
  uint64_t launches_lane;   /* one lane per message (k_digest_batch / k_digest_uniform) */
  uint64_t launches_pipe;   /* software-pipelined lane kernel (k_digest_*_pipe), <= 1 wave/SIMD */
  uint64_t launches_coop;   /* cooperative chaining (k_digest_coop) */
  uint64_t launches_split;  /* split chaining (k_digest_split, arena or digest-of-digests) */
  uint64_t launches_dod;    /* digest-of-digests, unsplit (k_digest_of_digests) */
  uint64_t split_retries;   /* host-call shards whose split launch timed out and were re-run unsplit */
  /* Last host-memory call, summed over GPUs (see msha_get_shard_stats): */
  uint64_t h2d_bytes;       /* payload + metadata uploaded */
  uint64_t d2h_bytes;       /* digests + status words downloaded */
  uint64_t small_calls;     /* host calls served by the small-call (latency) path: one H2D, one launch, one D2H */
  uint64_t staged_calls;    /* host calls whose pageable arena had the direct path's shape (16-B aligned,
                               dense): its touched runs went up through pinned staging, lanes planned
                               on the GPU (ABI 6) */
  uint64_t planned_device_calls; /* msha_digest_batch_device_planned calls (ABI 7) */
  /* Of launches_coop, the ones that ran a chain kernel (ABI 10): */
  uint64_t launches_chain2; /* two lanes a message (k_digest_chain2): late/host heads, small AUTO launches */
  uint64_t launches_chain8; /* eight lanes a message (k_digest_chain8): the folded early head, small launches */
  uint64_t small_zc_calls;  /* of small_calls, those served zero-copy: the kernel read the packed list and wrote
                               the digests in coherent pinned memory, no H2D or D2H (ABI 10) */
  uint64_t launches_lane_ws; /* of launches_lane, the work-stealing lane kernel (k_digest_batch_ws: folded
                                planned calls; ABI 10) */
} msha_stats;

/* Per-GPU figures of the last host-memory call (one entry per shard; a shard is
 * one GPU, or one virtual shard under MSHA_VIRTUAL_SHARDS). Times are
 * milliseconds since the call began. */
typedef struct {
  int32_t device;              /* HIP device id */
  uint32_t head_lanes;         /* pinned arenas: long chains run as heads (two-lane chain kernel, CUs of
                                  their own, payloads uploaded first; ABI 8) */
  uint64_t messages;           /* messages of this shard */
  uint64_t lanes;              /* distinct payloads hashed (aliases fold) */
  uint64_t h2d_payload_bytes;  /* message bytes uploaded (compacted byte ranges or staged chunks) */
  uint64_t h2d_bytes;          /* payload + metadata */
  uint64_t d2h_bytes;
  uint64_t launches;           /* kernel launches */
  double gather_begin_ms;      /* pageable arenas: first / last gather into pinned staging */
  double gather_end_ms;
  double gather_ms;            /* time spent gathering (sum over chunks) */
  double device_ms;            /* first H2D (metadata or payload) starts .. last kernel ends (HIP
                                  events on the shard's copy and compute streams) */
  double upload_ms;            /* first H2D starts .. last payload H2D ends: h2d_bytes / upload_ms
                                  is the shard's achieved PCIe rate */
  double kernel_ms;            /* first hash kernel starts .. last kernel ends */
  double first_launch_ms;      /* host: call start .. the shard's first hash kernel enqueued */
  double plan_kernel_ms;       /* pinned arenas: the GPU lane planner's kernels (plan.hip) */
} msha_shard_stats;

uint32_t msha_abi_version(void);

/* The build this library is: "src=<16 hex>;flags=<compile flags>", where src is
 * a hash of the sources it was compiled from (mirbft_amd/csrc/Makefile). A test
 * log names the build it ran with it; tests/conftest.py refuses a GPU session
 * whose library is not the tree's own (an experiment's build left in place).
 * Diagnostic, no reference counterpart (ABI 9). */
const char* msha_build_id(void);

/* Number of visible HIP devices (0 when none). */
int msha_device_count(int* n);

/* Create a context on the devices in device_mask (bit i = HIP device i);
 * device_mask == 0 means "device 0". Independent actions are sharded across
 * the masked devices (one stream per device, partitioned by cumulative block
 * count); no inter-GPU collective is used.
 * On failure the reason is written, NUL-terminated, into errbuf (when errbuf
 * is not NULL and errbuf_len > 0): the error travels with the call, so a
 * caller whose thread may change between two calls (a goroutine) still gets it. */
int msha_ctx_create_err(uint32_t device_mask, msha_ctx** out, char* errbuf, uint64_t errbuf_len);
/* The same; the reason of the most recent failed creation in the PROCESS is
 * then readable through msha_last_error(NULL) (prefer msha_ctx_create_err when
 * several threads create contexts). */
int msha_ctx_create(uint32_t device_mask, msha_ctx** out);
void msha_ctx_destroy(msha_ctx* ctx);
/* The context's last failure (ctx == NULL: the last failed creation). The
 * pointer stays valid for the context's life, but another thread's failing call
 * on the same context may rewrite the text while it is read: read it only while
 * no other call runs on the context, or use msha_last_error_copy. */
const char* msha_last_error(const msha_ctx* ctx);
/* Copy of the same text into buf (NUL-terminated, truncated to buf_len - 1),
 * taken under the context's lock: safe while other threads use the context.
 * Returns the text's full length. */
uint64_t msha_last_error_copy(const msha_ctx* ctx, char* buf, uint64_t buf_len);
int msha_get_stats(const msha_ctx* ctx, msha_stats* out);
/* Shards of the context (GPUs in device_mask, or virtual shards). */
int msha_shard_count(const msha_ctx* ctx, uint32_t* n);
int msha_get_shard_stats(const msha_ctx* ctx, uint32_t shard, msha_shard_stats* out);

/*
 * ProcessHashActions over a packed arena (serial.go:180-198).
 *   part j           = arena[part_off[j] : part_off[j] + part_len[j]]
 *   action i's parts = parts [action_part_begin[i], action_part_begin[i+1])
 *   out[32*i ...]    = SHA-256(concatenation of action i's parts)
 * Zero-part actions hash the empty string; empty parts contribute nothing;
 * parts may overlap or repeat. action_part_begin has n_actions+1 entries,
 * non-decreasing, action_part_begin[0] == 0, last == n_parts.
 */
int msha_hash_actions(msha_ctx* ctx, const uint8_t* arena, uint64_t arena_len,
                      const uint64_t* part_off, const uint64_t* part_len, uint64_t n_parts,
                      const uint64_t* action_part_begin, uint64_t n_actions, uint8_t* out);

/*
 * One-part messages (request digests, clients.go:189-192; or any action whose
 * parts the caller already concatenated): out[32*i] = SHA-256(arena[off[i] :
 * off[i]+len[i]]). Several messages may alias one payload (EpochChange
 * re-hashing, epoch_target.go:486-505): it is copied to the device once.
 */
int msha_digest_batch(msha_ctx* ctx, const uint8_t* arena, uint64_t arena_len,
                      const uint64_t* off, const uint64_t* len, uint64_t n, uint8_t* out);

/*
 * Batch / VerifyBatch digest over request-ack digests (sequence.go:155-158,
 * batch_tracker.go:175-178) when every part is a 32-byte digest:
 *   out[32*i] = SHA-256(table[idx[k]] for k in [begin[i], begin[i+1]))
 * table is n_table x 32 bytes; begin has n+1 entries.
 */
int msha_digest_of_digests(msha_ctx* ctx, const uint8_t* table, uint64_t n_table,
                           const uint32_t* idx, uint64_t n_idx, const uint64_t* begin,
                           uint64_t n, uint8_t* out);

/*
 * Device-resident (kernel-resident) forms, for callers that keep inputs in
 * HBM: every pointer is device memory on the context's FIRST device and the
 * work is enqueued on `stream` (a hipStream_t, NULL = the context's own
 * stream); the call returns after enqueueing. Arena rules: message starts
 * MSHA_DEVICE_ALIGN-aligned, MSHA_DEVICE_ARENA_SLACK readable bytes after the
 * last message. A misaligned start is reported by msha_device_status() and its
 * digest is zeroed (never a wrong digest). d_order (may be NULL) is a
 * permutation of [0, n): lane i hashes message d_order[i] (digest still lands
 * at d_out + 32*d_order[i]); pass msha_order_by_blocks()'s output for batches
 * of mixed sizes so every wavefront's lanes run the same number of blocks.
 */
int msha_digest_batch_device(msha_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_off,
                             const uint64_t* d_len, const uint32_t* d_order, uint64_t n,
                             uint8_t* d_out, void* stream);
/*
 * The same messages, planned on the GPU inside the call's own launches (no host
 * round trip, nothing precomputed by the caller): lanes are ordered by
 * descending block count; with MSHA_PLAN_FOLD_ALIASES, messages with equal
 * (d_off, d_len) -- EpochChange payloads re-hashed N^2 times,
 * epoch_target.go:486-505 -- are hashed once and the digest copied to every
 * such slot; and the longest chains, when one alone would outlast the rest of
 * the launch (a mixed storm sharded over several GPUs), run on the cooperative
 * kernel beside the lane kernel (a side stream forked from and joined back to
 * `stream`). Same arena rules and error reporting as msha_digest_batch_device;
 * n < 2^31. Returns after enqueueing. Not capturable into a HIP graph: the
 * call orders itself after the previous planned call through a library event
 * and forks to a library-owned stream, so on a capturing stream it fails with
 * MSHA_ERR_INVALID_ARG (msha_digest_batch_device captures).
 */
enum { MSHA_PLAN_FOLD_ALIASES = 1u };
int msha_digest_batch_device_planned(msha_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_off,
                                     const uint64_t* d_len, uint64_t n, uint32_t flags, uint8_t* d_out,
                                     void* stream);
/*
 * The plan of the last msha_digest_batch_device_planned call of the context (ABI 10,
 * additive: MSHA_HAS_PLANNED_READ tells a build that has it). Diagnostic, synchronous,
 * like msha_parts_plan_read_order: waits for the device, then copies the planner's
 * counters into *out, the lane order (message indices, position 0 first, 0xFFFFFFFF at
 * the `n - lanes` positions past the last lane) into order[0 .. min(n, order_cap)) and the
 * early head's list into longs[0 .. min(long_listed, long_cap, longs_cap)). order and longs
 * may be NULL when their cap is 0. Before any planned call: MSHA_OK with out->n == 0.
 * The lanes are ordered by descending class (exact length below 1 KiB, exact block count
 * below 4,096 blocks, floor(log2 blocks) above); inside a class any order may come back.
 */
#define MSHA_HAS_PLANNED_READ 1
typedef struct {
  uint64_t n;            /* messages of the last planned call; 0: none yet */
  uint32_t folded;       /* it had MSHA_PLAN_FOLD_ALIASES */
  uint32_t lanes;        /* messages that are hashed: order[0 .. lanes) */
  uint32_t head;         /* positions at the front the lane kernel skips: the head kernel's */
  uint32_t early;        /* the early head's lanes (0: none, or it stood down) */
  uint32_t late;         /* the late head's lanes (0 when the early head has the long lanes) */
  uint32_t long_lanes;   /* lanes of >= 256 blocks, as the scan counted them */
  uint32_t long_listed;  /* distinct long payloads the early head's pass listed */
  uint32_t gate;         /* the early head's first decision (0: it stood down before listing) */
  uint32_t long_cap, head_cap, head_per_wg;  /* what the call gave its kernels: the early head's
                            and the head's most lanes (long_cap 0: no early head was tried),
                            and the messages of one head workgroup */
  uint64_t gave_up;      /* tile look-backs that gave up waiting (folded calls; else 0) */
} msha_planned_plan;
int msha_planned_read_plan(msha_ctx* ctx, msha_planned_plan* out, uint32_t* order, uint64_t order_cap,
                           uint32_t* longs, uint64_t longs_cap);
/* Uniform layout: message i = d_arena[i*stride : i*stride + msg_len] (stride a
 * multiple of 16; messages may overlap, stride 0 hashes one message n times). */
int msha_digest_uniform_device(msha_ctx* ctx, const uint8_t* d_arena, uint64_t stride,
                               uint64_t msg_len, uint64_t n, uint8_t* d_out, void* stream);
int msha_digest_of_digests_device(msha_ctx* ctx, const uint8_t* d_table, const uint32_t* d_idx,
                                  const uint64_t* d_begin, uint64_t n, uint8_t* d_out,
                                  void* stream);
/* Synchronizes the context's first device and reports (then clears) any
 * device-side error flag raised by *_device calls: MSHA_OK, MSHA_ERR_ALIGNMENT,
 * MSHA_ERR_HIP if a split-chaining handoff (kernels.hip) waited over 100 ms, or
 * MSHA_ERR_INVALID_ARG for a decreasing part range given to msha_hash_actions_device
 * (reported after the other two when several are raised). */
int msha_device_status(msha_ctx* ctx);

/*
 * Kernel policy for one-part messages (msha_digest_batch, msha_hash_actions,
 * msha_digest_batch_device). Results are identical under every policy.
 *  MSHA_KERNEL_AUTO  (default) one lane per message when a launch has enough
 *                    messages to give every SIMD a wavefront; otherwise
 *                    cooperative chaining
 *  MSHA_KERNEL_LANE  always one wavefront lane per message
 *  MSHA_KERNEL_COOP  always cooperative chaining: per 64 messages a producer
 *                    wavefront expands the message schedules into LDS while a
 *                    consumer wavefront runs only the rounds (lower latency per
 *                    message; for few, large messages)
 */
enum { MSHA_KERNEL_AUTO = 0, MSHA_KERNEL_LANE = 1, MSHA_KERNEL_COOP = 2 };
int msha_set_kernel_policy(msha_ctx* ctx, int policy);

/*
 * Diagnostics (ABI 8): the clock the context's first GPU holds under the hash
 * kernels' instruction mix. A probe kernel compresses register-resident blocks
 * at the lane kernel's occupancy (8 waves per SIMD) and stamps s_memtime (shader
 * clock) and s_memrealtime (100 MHz) at each workgroup's start and end; the
 * clock is their ratio. Synchronous; run it right after the work whose clock
 * matters (the hash kernels carry no stamps). blocks_per_lane in [1, 100000]
 * (48: about 1 ms).
 */
typedef struct {
  double ghz_median;     /* over workgroups */
  double ghz_min;
  double ghz_max;
  double kernel_ms;      /* the probe launch, HIP events */
  double gblocks_per_s;  /* register-resident compression rate of the probe */
  uint32_t workgroups;
  uint32_t blocks_per_lane;
} msha_clock_info;
int msha_clock_probe(msha_ctx* ctx, uint32_t blocks_per_lane, msha_clock_info* out);

/* Pinned host memory for callers that want zero-copy staging: when the arena
 * passed to msha_digest_batch lies in such memory, every message start is
 * 16-byte aligned and the messages are packed without large gaps, each GPU's
 * byte span of it is DMA'd as is (no gather copy into the library's staging).
 * On a context whose GPUs sit on several NUMA nodes the allocation is cut into
 * one region per shard, in shard order, each placed on its GPU's node and
 * page-locked with hipHostRegister (MSHA_PINNED_STRIPE=1 forces, =0 disables):
 * a batch packed in message order then feeds each GPU from its own socket. */
int msha_pinned_alloc(msha_ctx* ctx, uint64_t bytes, void** p);
int msha_pinned_free(msha_ctx* ctx, void* p);

/*
 * Stream sets: many resumable SHA-256 streams with hash.Hash semantics, the
 * streaming half of processor.Hasher (New() hash.Hash, pkg/processor/serial.go:21-23):
 * Write appends, Sum(b) appends the digest of everything written so far and
 * changes nothing. The reference streams in NodeState (pkg/testengine/recorder.go:
 * 288-359: Apply writes each committed digest into ActiveHash as it arrives, Snap
 * takes Sum(nil) and starts a new hash from it); the same shape serves per-client
 * running hashes, or a message set whose bytes arrive in pieces or do not fit one
 * arena. The GPU gains from parallelism ACROSS streams: one stream is one lane,
 * so a lone stream runs at one lane's rate (tens of MB/s). ABI 10, additive:
 * MSHA_HAS_STREAMS tells a build that has them.
 *
 * A set keeps, per stream, the 8-word chaining state on the context's first
 * device and, on the host, the byte count and the buffered tail of fewer than 64
 * bytes; the GPU never sees a partial block. A set must be destroyed before its
 * context; calls on it take the context's lock. After a HIP error a set is
 * failed: every call returns MSHA_ERR_HIP until msha_streams_reset(set, NULL, 0).
 * There is no CPU fallback: Sum runs on the GPU as well.
 */
#define MSHA_HAS_STREAMS 1
/* Bytes of one exported stream: "sha\x03", the 8 state words big-endian, 64
 * buffer bytes (zero past length % 64), the length as a big-endian uint64. The
 * layout is meant to equal Go crypto/sha256's MarshalBinary
 * (encoding.BinaryMarshaler), so a half-hashed state could pass between this
 * engine and a Go hash.Hash; with no Go toolchain where this was built that
 * equality is UNVERIFIED. */
#define MSHA_STREAM_STATE_BYTES 108u
typedef struct msha_streams msha_streams;
/* n streams in New() state (recorder.go:420, Hasher.New()) on the context's first
 * device. staging_bytes bounds the pinned and device staging one piece of a write
 * may use (0: 64 MiB; min 4096; rounded to 64): memory stays bounded by it
 * whatever a call's size. n < 2^32. */
int msha_streams_create(msha_ctx* ctx, uint64_t n, uint64_t staging_bytes, msha_streams** out);
void msha_streams_destroy(msha_streams* set);
/* Write (hash.Hash.Write; recorder.go:348, ActiveHash.Write(digest)): for j in call
 * order, stream id[j] appends arena[off[j] : off[j]+len[j]]. An id may repeat; its
 * chunks append in order. Everything is validated first (ids below n, ranges
 * inside the arena): a bad argument returns MSHA_ERR_INVALID_ARG and changes no
 * stream. A call that leaves every touched stream under one block launches
 * nothing. */
int msha_streams_write(msha_streams* set, const uint8_t* arena, uint64_t arena_len,
                       const uint64_t* id, const uint64_t* off, const uint64_t* len, uint64_t k);
/* Sum(nil) (recorder.go:298): out[32 j] = SHA-256 of everything written to id[j];
 * no stream changes. id NULL: all n streams, k == n. */
int msha_streams_sum(msha_streams* set, const uint64_t* id, uint64_t k, uint8_t* out);
/* Reset (hash.Hash.Reset; recorder.go:299, a new hash per checkpoint): the streams
 * return to New() state. id NULL: all, and a failed set is usable again. */
int msha_streams_reset(msha_streams* set, const uint64_t* id, uint64_t k);
/* out[j] = bytes written to id[j] so far (id NULL: all n streams, k == n). */
int msha_streams_length(const msha_streams* set, const uint64_t* id, uint64_t k, uint64_t* out);
/* MarshalBinary / UnmarshalBinary of the streams id[j] (id NULL: all, k == n):
 * k x MSHA_STREAM_STATE_BYTES bytes. Import ignores buffer bytes past length % 64
 * and rejects a wrong magic (MSHA_ERR_INVALID_ARG, no stream changed). An id
 * repeated in one import is sequential UnmarshalBinary: the last entry wins for
 * state, buffer and length alike. */
int msha_streams_export(msha_streams* set, const uint64_t* id, uint64_t k, uint8_t* out);
int msha_streams_import(msha_streams* set, const uint64_t* id, uint64_t k, const uint8_t* in);
typedef struct {
  uint64_t writes;               /* msha_streams_write calls completed */
  uint64_t sums;                 /* msha_streams_sum calls completed */
  uint64_t bytes_written;
  uint64_t blocks_absorbed;      /* whole blocks compressed by the absorb kernel */
  uint64_t blocks_finished;      /* tail and length blocks compressed by the finish kernel */
  uint64_t launches_absorb;
  uint64_t launches_finish;
  uint64_t buffered_only_writes; /* writes that launched nothing (every touched stream under one block) */
  uint64_t pieces;               /* staging pieces uploaded by writes */
  uint32_t last_load_mode;       /* load mode of the last absorb / finish launch (1 prefetch, 2 paired) */
  uint32_t last_lanes;           /* its lanes */
  double last_kernel_ms;         /* its kernel time (HIP events) */
} msha_streams_stats;
int msha_streams_get_stats(const msha_streams* set, msha_streams_stats* out);
/*
 * Device-resident forms of the two primitives the sets run on, same rules as
 * msha_digest_batch_device (device memory of the context's first device, starts
 * MSHA_DEVICE_ALIGN-aligned, MSHA_DEVICE_ARENA_SLACK readable bytes after the last
 * lane's bytes, errors through msha_device_status); they return after enqueueing.
 * Absorb (Write of whole blocks): lane i compresses d_nblocks[i] 64-byte blocks at
 * d_arena + d_off[i] into d_state[8 i .. 8 i + 8) (host-order words, in/out; a New()
 * stream holds the FIPS 180-4 initial value). A lane with no block, or with a
 * misaligned start, leaves its state as it was.
 * Finish (Sum): d_out[32 i] = the digest of a message whose first d_prefix[i]
 * bytes (a multiple of 64; NULL: 0) are in d_state[8 i ..] (NULL: the initial
 * value) and whose last d_len[i] bytes are at d_arena + d_off[i]; the state is not
 * written. With both NULL this is msha_digest_batch_device.
 */
int msha_absorb_device(msha_ctx* ctx, uint32_t* d_state, const uint8_t* d_arena,
                       const uint64_t* d_off, const uint64_t* d_nblocks, uint64_t n, void* stream);
int msha_finish_device(msha_ctx* ctx, const uint32_t* d_state, const uint64_t* d_prefix,
                       const uint8_t* d_arena, const uint64_t* d_off, const uint64_t* d_len, uint64_t n,
                       uint8_t* d_out, void* stream);
/*
 * Absorb on the eight-lane chain (ABI 10, additive: MSHA_HAS_ABSORB_CHAIN tells a build
 * that has it). The contract is msha_absorb_device's, word for word: the same arguments,
 * device memory of the context's first device, starts MSHA_DEVICE_ALIGN-aligned,
 * MSHA_DEVICE_ARENA_SLACK readable bytes after the last lane's bytes, errors through
 * msha_device_status, the same host checks, n == 0 launches nothing; a lane with no
 * block, or with a misaligned start (reported once), leaves its state as it was; and the
 * states afterwards are bit for bit msha_absorb_device's. What differs is the kernel:
 * msha_absorb_device gives a lane one GPU lane, so a lone long lane runs at one lane's
 * rate; here a lane is eight GPU lanes and a share of two producer waves, the round
 * engine of the eight-lane digest chain resumed from the given state and stopped
 * without padding. It is for FEW, LONG lanes: 16 lanes a workgroup, one workgroup a
 * compute unit, so beyond 16 x compute units lanes the workgroups queue
 * (profiles/streams_device/README.md says where it stops paying). One launch on
 * `stream` (NULL: the context's own), no host wait: capturable. No block is read past a
 * lane's last. msha_set_kernel_policy does not apply. The launch counts in msha_stats
 * as every chain launch does: launches_coop and launches_chain8.
 */
#define MSHA_HAS_ABSORB_CHAIN 1
int msha_absorb_chain_device(msha_ctx* ctx, uint32_t* d_state, const uint8_t* d_arena,
                             const uint64_t* d_off, const uint64_t* d_nblocks, uint64_t n, void* stream);

/*
 * Device stream sets: the stream sets above with everything in device memory (ABI 10,
 * additive: MSHA_HAS_STREAMS_DEVICE tells a build that has them). NodeState.Apply
 * (pkg/testengine/recorder.go:333-359) writes each committed request digest into
 * ActiveHash, and Snap (recorder.go:288-300) takes Sum(nil), starts a new hash and
 * writes the sum into it. When those digests are produced in HBM
 * (msha_digest_batch_device), a host set costs a copy down, a repack, a copy up and a
 * wait per call; msha_absorb_device / msha_finish_device take whole 16-byte aligned
 * blocks only and leave the partial-block bookkeeping to the host. Here a stream's
 * chaining state, its 64-byte buffer (bytes past length % 64 always zero) and its
 * 64-bit length all live on the context's first device, allocated once in create.
 *
 * Write, Sum, Snap and Reset are DEVICE CALLS: every pointer is device memory of the
 * context's first device, `stream` NULL means the context's own stream, and the call
 * returns after enqueueing exactly one kernel launch -- no memset, no library stream,
 * no event wait, no allocation -- so it captures into a HIP graph as one kernel node
 * (a replayed write appends again). n_rows == 0 returns MSHA_OK and launches nothing.
 * (msha_dstreams_write_jobs_device, further down, is the exception: several launches.)
 * Ordering between calls on different HIP streams is the caller's. A set must be
 * destroyed before its context; calls on it take the context's lock.
 *
 * Rows. Row r of a call, r in [0, n_rows), is stream s = d_row ? d_row[r] : r (d_row
 * NULL: n_rows must equal n, checked here). A stream may be named AT MOST ONCE per
 * call, the rule of the host sets' row kernels; a repeat is NOT detected: that stream
 * alone is left in an unspecified state, no other stream is affected and nothing is
 * read or written outside the set's memory. A stream's chunks of one call go into one
 * row's part list, which is what the CSR d_row_part_begin (n_rows + 1 entries) is for.
 *
 * Write (hash.Hash.Write; recorder.go:348): row r appends the parts
 * [d_row_part_begin[r], d_row_part_begin[r+1]) back to back,
 *   part j = d_arena[d_part_off[j] : d_part_off[j] + d_part_len[j]].
 * The arena rules are the READ CONTRACT of msha_hash_actions_device below: a part may
 * start at any byte and have any length; only address-aligned 16-byte granules that
 * hold a byte of a non-empty part are read; d_arena must be 16-byte aligned (checked
 * here: MSHA_ERR_INVALID_ARG); MSHA_DEVICE_ARENA_SLACK readable bytes must follow the
 * last part. Part offsets are below 2^63 (bit 63 marks the stream's own buffer inside
 * the kernel; an offset that carries it reads that buffer, never other memory). Empty
 * parts and zero-part rows contribute nothing; a row that appends nothing stores
 * nothing.
 *
 * Checked on the host (MSHA_ERR_INVALID_ARG with a text): null pointers, d_arena's
 * alignment, n_rows >= 2^32 - 1, d_row NULL with n_rows != n, an import with a wrong
 * magic. Reported by msha_device_status(), once, for what the host cannot see:
 *  - d_row[r] >= n: no stream is touched, Sum and Snap zero that d_out row, and a bit
 *    of its own (32) is raised in the device error word: MSHA_ERR_INVALID_ARG
 *    ("msha_dstreams_*: row out of range ..."), appended to an older bit's text when
 *    one is raised too;
 *  - a row whose part range decreases (or spans 2^32 parts or more): the stream is
 *    unchanged, and the bit and text of msha_hash_actions_device's decreasing
 *    action_part_begin are raised.
 */
#define MSHA_HAS_STREAMS_DEVICE 1
typedef struct msha_dstreams msha_dstreams;
/* n streams in New() state (recorder.go:420, Hasher.New()); n in [1, 2^32 - 1). */
int msha_dstreams_create(msha_ctx* ctx, uint64_t n, msha_dstreams** out);
void msha_dstreams_destroy(msha_dstreams* set);
int msha_dstreams_write_device(msha_dstreams* set, const uint8_t* d_arena,
                               const uint64_t* d_part_off, const uint64_t* d_part_len,
                               const uint64_t* d_row_part_begin, const uint32_t* d_row,
                               uint64_t n_rows, void* stream);
/* Sum(nil) (recorder.go:298): d_out[32 r] = SHA-256 of everything written to row r's
 * stream; no stream changes. */
int msha_dstreams_sum_device(msha_dstreams* set, const uint32_t* d_row, uint64_t n_rows,
                             uint8_t* d_out, void* stream);
/* Snap (recorder.go:298-300): d_out[32 r] = Sum(nil); then the stream is New()
 * followed by Write(that sum): 32 bytes buffered, length 32. */
int msha_dstreams_snap_device(msha_dstreams* set, const uint32_t* d_row, uint64_t n_rows,
                              uint8_t* d_out, void* stream);
/* Reset (hash.Hash.Reset): the rows' streams return to New(). */
int msha_dstreams_reset_device(msha_dstreams* set, const uint32_t* d_row, uint64_t n_rows,
                               void* stream);
/* Synchronous, host memory: these wait for the device (everything enqueued on it so
 * far), then read or replace whole streams; id NULL: all n streams, k == n; an id >= n
 * is MSHA_ERR_INVALID_ARG. Export and import use the MSHA_STREAM_STATE_BYTES layout of
 * msha_streams_export, so a state moves freely between a host set and a device set.
 * Import ignores buffer bytes past length % 64 (they are stored as zeros) and rejects
 * a wrong magic with no stream changed; of the entries naming one stream the last
 * wins, as in msha_streams_import. */
int msha_dstreams_length(msha_dstreams* set, const uint64_t* id, uint64_t k, uint64_t* out);
int msha_dstreams_export(msha_dstreams* set, const uint64_t* id, uint64_t k, uint8_t* out);
int msha_dstreams_import(msha_dstreams* set, const uint64_t* id, uint64_t k, const uint8_t* in);
typedef struct {
  uint64_t writes;        /* device calls that enqueued their launch, by kind */
  uint64_t sums;
  uint64_t snaps;
  uint64_t resets;
  uint64_t launches;      /* kernel launches of those calls: one each */
  uint64_t last_rows;     /* rows of the last one */
  double last_kernel_ms;  /* its kernel time by HIP events, measured only under MSHA_PARTS_TIMING=1
                             (the call then waits for the kernel; never while `stream` is being
                             captured); otherwise 0 and the call stays enqueue-only */
} msha_dstreams_stats;
int msha_dstreams_get_stats(const msha_dstreams* set, msha_dstreams_stats* out);

/*
 * Write jobs in call order: msha_streams_write's job list in device memory (ABI 10,
 * additive: MSHA_HAS_STREAMS_DEVICE_JOBS tells a build that has it). NodeState.Apply
 * (recorder.go:333-359) makes its Write calls in commit order, every node every
 * digest as it arrives; a caller that learns on the device which stream takes which
 * chunk holds that order, not the CSR grouped by stream that
 * msha_dstreams_write_device wants. Here, for j = 0 .. n_jobs-1 in that order,
 *   stream d_job_stream[j] appends d_arena[d_job_off[j] : d_job_off[j] + d_job_len[j]].
 * A stream may be named any number of times; its chunks append in job order; empty
 * chunks contribute nothing. The result is bit for bit what msha_dstreams_write_device
 * produces for the same jobs grouped stably by stream: state, buffer and length.
 *
 * The grouping is done on the GPU inside the call: a stable radix sort of (min(stream,
 * n), j), 8 bits a pass, ceil(bit_width(n) / 8) passes of three kernels each, two
 * kernels that turn the order into the CSR, then msha_dstreams_write_device's kernel
 * over all n streams. So, UNLIKE the four device calls above, this one enqueues
 * SEVERAL kernel launches, 3 * passes + 3, all of them on `stream` (NULL: the
 * context's own), still with no memset, no library stream and no host wait; it
 * captures into a HIP graph as a chain of kernel nodes (a replay appends again). No
 * kernel waits on another workgroup. n_jobs == 0 returns MSHA_OK and launches nothing.
 *
 * The arena rules are msha_dstreams_write_device's (the READ CONTRACT of
 * msha_hash_actions_device): any start, 16-byte aligned d_arena,
 * MSHA_DEVICE_ARENA_SLACK readable bytes behind the last chunk, offsets below 2^63.
 * d_job_off[j] and d_job_len[j] are read for every job; arena bytes only for valid
 * jobs. A job whose stream is >= n is DROPPED: no stream is touched by it, its chunk is
 * not read, every other job of the call is applied exactly, and msha_device_status()
 * reports msha_dstreams_*'s row out of range (bit 32), once. Checked on the host
 * (MSHA_ERR_INVALID_ARG with a text, no stream changed): null pointers, d_arena's
 * alignment, n_jobs >= 2^32 - 1.
 *
 * The workspace (about 32.5 bytes a job and 8 (n + 1)) belongs to the set and is freed
 * in destroy. It grows, by hipMalloc, only while `stream` is not being captured, after
 * waiting for the set's previous jobs call; on a capturing stream a workspace that is
 * too small is MSHA_ERR_INVALID_ARG: make one call of that size outside the capture
 * first. Outside capture a call is ordered after the set's previous jobs call through
 * an event, so two HIP streams do not race on the workspace; ordering against the
 * set's other calls is the caller's, as above.
 */
#define MSHA_HAS_STREAMS_DEVICE_JOBS 1
int msha_dstreams_write_jobs_device(msha_dstreams* set, const uint8_t* d_arena,
                                    const uint32_t* d_job_stream, const uint64_t* d_job_off,
                                    const uint64_t* d_job_len, uint64_t n_jobs, void* stream);
typedef struct {
  uint64_t calls;           /* jobs calls that enqueued their launches (msha_dstreams_stats counts none of them) */
  uint64_t jobs;            /* jobs of those calls */
  uint64_t launches_sort;   /* histogram, scan and scatter launches: 3 a pass */
  uint64_t launches_rows;   /* the two CSR kernels */
  uint64_t launches_write;  /* msha_dstreams_write_device's kernel: one a call */
  uint64_t last_passes;     /* radix passes of the last call: ceil(bit_width(n) / 8) */
  uint64_t last_jobs;
  uint64_t tile_jobs;       /* jobs a workgroup ranks per pass: a constant, valid from create */
  double last_kernel_ms;    /* all of the last call's kernels by HIP events, only under MSHA_PARTS_TIMING=1
                               (the call then waits for them; never while `stream` is being captured) */
} msha_dstreams_jobs_stats;
int msha_dstreams_get_jobs_stats(const msha_dstreams* set, msha_dstreams_jobs_stats* out);
/* Diagnostic, synchronous (waits for the device): the job order of the set's last jobs
 * call, position 0 first -- order[p] is the job applied p-th, jobs of one stream
 * adjacent and in call order, dropped jobs last -- up to cap entries; *n_jobs = that
 * call's job count, *n_valid = how many leading positions are valid jobs. It is
 * argsort(min(stream, n), stable) exactly. Before any jobs call both counts are 0. */
int msha_dstreams_jobs_read_order(msha_dstreams* set, uint32_t* order, uint64_t cap,
                                  uint64_t* n_jobs, uint64_t* n_valid);

/*
 * ProcessHashActions from HBM (serial.go:180-198), the device-resident form of
 * msha_hash_actions (ABI 10, additive: MSHA_HAS_PARTS_DEVICE tells a build that has
 * it). An action's Data is a list of byte slices hashed back to back; an
 * EpochChange's interleaves 8-byte big-endian fields with 32-byte digests
 * (stateless.go:323-352). Here the slices stay where they are in device memory:
 *   part j           = d_arena[d_part_off[j] : d_part_off[j] + d_part_len[j]]
 *   action i's parts = parts [d_action_part_begin[i], d_action_part_begin[i+1])
 *   d_out[32*i ...]  = SHA-256(concatenation of action i's parts)
 * A zero-part action hashes the empty string; empty parts contribute nothing; parts
 * may overlap, repeat and be shared between actions. Offsets and lengths are 64-bit
 * (an arena past 4 GiB, an action past 2^32 bytes); an action has fewer than 2^32
 * blocks and fewer than 2^32 parts. d_action_part_begin has n_actions + 1 entries. d_order (may be NULL) is as
 * in msha_digest_batch_device: lane i hashes action d_order[i], whose digest still
 * lands at d_out + 32*d_order[i].
 *
 * Every pointer is device memory of the context's FIRST device; the call returns
 * after enqueueing on `stream` (NULL: the context's own). It is one kernel launch, on
 * no library stream and with no host wait, so it can be captured into a HIP graph as
 * msha_digest_batch_device can.
 *
 * Arena rules, weaker than the other device entries' -- the READ CONTRACT:
 *  - a part may start at any byte and have any length;
 *  - the kernel reads only address-aligned 16-byte granules that contain at least
 *    one byte of a non-empty part, and nothing else of the arena (a part's
 *    neighbours inside its first and last granule are read and ignored);
 *  - d_arena itself must be 16-byte aligned (checked here: MSHA_ERR_INVALID_ARG), so
 *    that granules of offsets are granules of addresses;
 *  - MSHA_DEVICE_ARENA_SLACK readable bytes must follow the last part.
 * The host cannot see the device arrays. An action whose part range decreases
 * (begin[i+1] < begin[i]; or spans 2^32 parts or more) gets an all-zero digest, never a wrong one, and raises a
 * bit of its own in the device error word: msha_device_status() then returns
 * MSHA_ERR_INVALID_ARG ("... action_part_begin decreases ...") and clears it. Part
 * offsets and lengths are trusted, as the offsets of the other device entries are.
 */
#define MSHA_HAS_PARTS_DEVICE 1
int msha_hash_actions_device(msha_ctx* ctx, const uint8_t* d_arena,
                             const uint64_t* d_part_off, const uint64_t* d_part_len,
                             const uint64_t* d_action_part_begin, const uint32_t* d_order,
                             uint64_t n_actions, uint8_t* d_out, void* stream);
/* Counters of msha_hash_actions_device (msha_stats keeps its size). */
typedef struct {
  uint64_t calls;         /* calls that enqueued their launch */
  uint64_t actions;       /* digests they produce */
  uint64_t launches;      /* k_digest_parts launches */
  uint64_t last_lanes;    /* lanes of the last launch */
  double last_kernel_ms;  /* its kernel time by HIP events, measured only under MSHA_PARTS_TIMING=1
                             (the call then waits for the kernel; never while `stream` is being
                             captured); otherwise 0 and the call stays enqueue-only */
} msha_parts_stats;
int msha_get_parts_stats(const msha_ctx* ctx, msha_parts_stats* out);

/*
 * Multi-part actions through part LISTS, planned and folded on the GPU (ABI 10,
 * additive: MSHA_HAS_PARTS_PLANNED tells a build that has it). One more level of
 * indirection than msha_hash_actions_device, actions -> lists -> parts:
 *   list l           = parts [d_list_part_begin[l], d_list_part_begin[l+1])
 *   action i         hashes list d_action_list[i]  (d_action_list NULL: list i, and
 *                    n_actions must equal n_lists)
 *   d_out[32*i ...]  = SHA-256(the list's parts back to back)
 * Parts, the arena and d_out are as in msha_hash_actions_device, under its READ
 * CONTRACT (any byte offset, 16-byte granules, a 16-byte aligned d_arena,
 * MSHA_DEVICE_ARENA_SLACK readable bytes after the last part). d_list_part_begin has
 * n_lists + 1 entries; n_lists and n_actions are each below 2^32 - 1.
 *
 * FOLDING comes with the indirection: two actions are the same message exactly when
 * they name the same list (an integer compare: no contents are hashed or compared to
 * find that out). Every list named at least once is hashed exactly once, however many
 * actions name it. A list no action names is not hashed, and neither its entry of
 * d_list_part_begin nor its parts are read. `flags` is reserved (MSHA_PARTS_FOLD names
 * what is implied anyway); any other bit is MSHA_ERR_INVALID_ARG.
 *
 * ORDER: the lanes are the named lists, ordered on the GPU inside the call by
 * descending block-count class -- the exact block count below 4,096 blocks, powers of
 * two from there up, as msha_digest_batch_device_planned orders its lanes -- so the
 * lanes of a wave finish together. The order inside a class is unspecified.
 *
 * ERRORS the host cannot see are reported by msha_device_status(), once:
 *  - d_action_list[i] >= n_lists: action i gets an all-zero digest and bit 8 of the
 *    device error word is raised: MSHA_ERR_INVALID_ARG ("... action_list out of range
 *    ...");
 *  - a list whose part range decreases (or spans 2^32 parts or more): every action
 *    naming it gets an all-zero digest, and the bit msha_hash_actions_device raises for
 *    it (4) is raised: MSHA_ERR_INVALID_ARG ("... action_part_begin decreases ...").
 * Checked on the host (MSHA_ERR_INVALID_ARG): null pointers, d_arena's alignment,
 * unknown flags, the two counts' bound, n_actions != n_lists without d_action_list.
 * n_actions == 0 returns MSHA_OK and launches nothing.
 *
 * ONE STREAM, capturable: the kernels (init, mark, measure, scan, scatter, hash, fill)
 * all go on `stream` (NULL: the context's own); there is no memset, no library stream
 * and no host wait. The workspace (class keys, counters, the order, a used flag per list, and
 * with d_action_list the lists' digest table: 6 to 39 bytes a list) belongs to the
 * context and grows by hipMalloc only while `stream` is NOT being captured; growing
 * waits for the previous call. On a capturing stream with too small a workspace (or a
 * context that has made no device call yet) the call fails with MSHA_ERR_INVALID_ARG
 * and says to make one call of that size outside the capture first. Outside capture a
 * call is ordered after the previous planned-parts call of the context through a
 * library event, so calls on two streams do not race on the workspace. A captured call
 * holds the workspace's addresses: replaying it concurrently with another planned-parts
 * call on the same context is the caller's to order, and a later call that grows the
 * workspace invalidates it.
 */
#define MSHA_HAS_PARTS_PLANNED 1
enum { MSHA_PARTS_FOLD = 1u };
int msha_hash_actions_device_planned(msha_ctx* ctx, const uint8_t* d_arena,
                                     const uint64_t* d_part_off, const uint64_t* d_part_len,
                                     const uint64_t* d_list_part_begin, uint64_t n_lists,
                                     const uint32_t* d_action_list, uint64_t n_actions,
                                     uint32_t flags, uint8_t* d_out, void* stream);
/* Counters of msha_hash_actions_device_planned (msha_stats and msha_parts_stats are
 * untouched by it). */
typedef struct {
  uint64_t calls;          /* calls that enqueued their launches */
  uint64_t actions;        /* digests they produce */
  uint64_t lists;          /* lists they were given */
  uint64_t last_lanes;     /* the last call's distinct lists hashed ... */
  uint64_t last_blocks;    /* ... and the 64-byte blocks compressed for them; both read back, and */
  uint64_t launches_plan;  /* init, mark, measure, scan and scatter launches */
  uint64_t launches_hash;  /* k_digest_parts_planned launches */
  uint64_t launches_fill;  /* k_parts_fill launches (calls with d_action_list) */
  double last_kernel_ms;   /* the call's kernels timed by HIP events, only under MSHA_PARTS_TIMING=1
                              (read at each call; the call then waits for its kernels; never while
                              `stream` is being captured); otherwise these three are 0 */
} msha_parts_plan_stats;
int msha_get_parts_plan_stats(const msha_ctx* ctx, msha_parts_plan_stats* out);
/* Diagnostic, synchronous: waits for the device, then copies the last call's lane order
 * (list indices, position 0 first) into order[0 .. min(cap, *lanes)) and its lane count
 * into *lanes. order may be NULL when cap is 0. */
int msha_parts_plan_read_order(msha_ctx* ctx, uint32_t* order, uint64_t cap, uint64_t* lanes);

/*
 * Part lists flattened on the GPU (ABI 10, additive: MSHA_HAS_PARTS_CONCAT tells a
 * build that has it). The parts kernels above walk a list on one lane; every other
 * device entry wants contiguous, MSHA_DEVICE_ALIGN-aligned messages. This entry turns
 * selected lists into such messages without a host round trip, so that a caller can
 * hand its long lists (an EpochChange: thousands of parts) to msha_digest_batch_device
 * and leave the short ones on msha_hash_actions_device_planned.
 *
 * MESSAGES. Message k, for k in [0, n_select), is list s = d_select[k]; with d_select
 * NULL message k is list k and n_select must equal n_lists. List s owns the parts
 * [d_list_part_begin[s], d_list_part_begin[s+1]) (n_lists + 1 entries), and part j is
 * d_arena[d_part_off[j] : d_part_off[j] + d_part_len[j]], as in
 * msha_hash_actions_device_planned. An id may repeat in d_select: each repeat is
 * another copy, a message of its own.
 *
 * LAYOUT. d_msg_len[k] is the sum of the list's part lengths, d_msg_off[0] = 0 and
 * d_msg_off[k+1] = d_msg_off[k] + round16(d_msg_len[k]): every start is
 * MSHA_DEVICE_ALIGN-aligned, messages come in k order, and there are no gaps beyond
 * the pad. d_msg_off and d_msg_len have n_select entries each.
 *
 * BYTES WRITTEN. d_dst[off[k] : off[k] + len[k]] holds the list's parts back to back,
 * and the pad up to round16(len[k]) is written as zeros. No other byte of d_dst is
 * written.
 *
 * FIT. Message k fits iff off[k] + round16(len[k]) + MSHA_DEVICE_ARENA_SLACK <=
 * dst_bytes: with that slack whatever the digest entries read past a message stays
 * inside d_dst, so (d_dst, d_msg_off, d_msg_len) can go to msha_digest_batch_device as
 * they are.
 *
 * NEVER AN UNSAFE LAYOUT. Three kinds of message are not written: one that does not
 * fit; one whose d_select[k] >= n_lists; one whose list's part range decreases or spans
 * 2^32 parts or more. Such a message gets d_msg_off[k] = d_msg_len[k] = 0 (the empty
 * message at d_dst's start), so nothing downstream reads outside d_dst. An invalid list
 * (the last two kinds) counts as length 0 in the running offset. A message that does
 * not fit counts with its length, so once one message does not fit, none after it does
 * either: all of them are refused, and every message before them is exact. Each of the
 * three raises bit 16 of the device error word: msha_device_status() then returns
 * MSHA_ERR_INVALID_ARG with a text that names msha_concat_lists_device and the three
 * causes, once, and clears it. Set together with an older bit, that bit's code and
 * text are reported unchanged and this clause is appended to them.
 *
 * READ CONTRACT: the one of msha_hash_actions_device. Only address-aligned 16-byte
 * granules that hold a byte of a non-empty part of a selected, valid list are read (a
 * refused list's parts are not read at all); d_list_part_begin[s] and [s+1] of lists
 * nobody selects are not read. Part offsets and lengths are trusted. d_dst must not
 * overlap the arena or any of the arrays: that is the caller's error and is not
 * detected.
 *
 * Checked on the host (MSHA_ERR_INVALID_ARG, each with a text): null pointers; d_arena
 * or d_dst not MSHA_DEVICE_ALIGN-aligned; n_lists or n_select at or above 2^32 - 1;
 * n_select != n_lists without d_select. n_select == 0 returns MSHA_OK and launches
 * nothing.
 *
 * ONE STREAM, capturable: three kernels (measure, scan, copy) go on `stream` (NULL: the
 * context's own). There is no memset, no library stream, no host wait and no workspace
 * of the context's -- between the first two kernels d_msg_off carries a flag -- so the
 * call captures into a HIP graph as a linear chain of three kernel nodes. The one
 * allocation is the context's error word on its first device call: on a capturing
 * stream a context that has made no device call yet fails with MSHA_ERR_INVALID_ARG
 * and says to make one call of this size outside the capture first.
 */
#define MSHA_HAS_PARTS_CONCAT 1
int msha_concat_lists_device(msha_ctx* ctx, const uint8_t* d_arena,
                             const uint64_t* d_part_off, const uint64_t* d_part_len,
                             const uint64_t* d_list_part_begin, uint64_t n_lists,
                             const uint32_t* d_select, uint64_t n_select,
                             uint8_t* d_dst, uint64_t dst_bytes,
                             uint64_t* d_msg_off, uint64_t* d_msg_len, void* stream);
/* Counters of msha_concat_lists_device (msha_stats, msha_parts_stats and
 * msha_parts_plan_stats are untouched by it). */
typedef struct {
  uint64_t calls;         /* calls that enqueued their launches */
  uint64_t lists;         /* messages they were asked for (n_select) */
  uint64_t launches;      /* kernel launches: three a call */
  uint64_t last_bytes;    /* the last call's last valid message's off + round16(len), read back, and */
  double last_kernel_ms;  /* its kernels timed by HIP events, only under MSHA_PARTS_TIMING=1 (read at
                             each call; the call then waits for its kernels; never while `stream` is
                             being captured); otherwise both are 0 */
} msha_concat_stats;
int msha_get_concat_stats(const msha_ctx* ctx, msha_concat_stats* out);

/*
 * Part lists with their long lists routed to the chains (ABI 10, additive:
 * MSHA_HAS_PARTS_ROUTED tells a build that has it). ProcessHashActions from HBM
 * (serial.go:180-198) once more, for batches in which a few lists are very long: an
 * EpochChange's Data (stateless.go:323-352) is thousands of parts, and as a lane of
 * msha_hash_actions_device_planned it holds its whole call up. This entry is that one
 * with the decision made on the GPU inside the call: it finds the long lists among the
 * named ones, flattens them as msha_concat_lists_device does and hashes them on the
 * eight-lane chain kernel, and hashes the rest as lanes. One call, and the caller need
 * not know which lists are long.
 *
 * SAME DIGESTS, SAME ERRORS as msha_hash_actions_device_planned. Lists, actions, d_out,
 * the READ CONTRACT and FOLDING (a named list is hashed exactly once; a list no action
 * names is never read) are that entry's, and so are both device error bits: bit 8 for a
 * d_action_list entry >= n_lists, bit 4 for a list whose part range decreases or spans
 * 2^32 parts or more, all-zero digests for either. Checked on the host
 * (MSHA_ERR_INVALID_ARG, each with a text): null pointers, d_arena's alignment, the two
 * counts' bound, n_actions != n_lists without d_action_list, and the bounds of `opts`
 * below. n_actions == 0 returns MSHA_OK and launches nothing; it is looked at after the
 * counts and before `opts` and the pointers, which such a call does not use. Routing is
 * an optimisation: no input makes a digest differ from the planned entry's, and nothing
 * here raises bit 16 (msha_concat_lists_device's).
 *
 * WHAT IS ROUTED. A list is LONG when some action names it, its part range is valid and
 * msha_blocks_for_len(the sum of its part lengths) >= long_blocks. A long list that
 * finds a slot and room is routed: its parts are written back to back, from a
 * MSHA_DEVICE_ALIGN-aligned start and with a zeroed pad, into a flatten buffer the
 * context owns, and it is hashed from there by the eight-lane chain kernel; it is not a
 * lane of the parts kernel. msha_set_kernel_policy does not apply: the routed lists
 * always run on that kernel, 16 lists a compute unit, which is why max_long is capped.
 *
 * CAPS NEVER FAIL A CALL. At most max_long lists are routed, and a list is given room
 * only while off + round16(len) + MSHA_DEVICE_ARENA_SLACK <= long_bytes holds for it
 * (off: the rounded lengths of the lists given room before it). A long list that finds
 * no slot or no room stays an ordinary lane and its digest is as right as any. When
 * every long list fits both caps, exactly the long lists are routed. When not all fit,
 * which of them are routed is unspecified, but of long lists of one length L exactly
 * min(n_long, max_long, floor((long_bytes - MSHA_DEVICE_ARENA_SLACK) / round16(L)))
 * are.
 *
 * DEFAULTS (a zero field, or opts NULL). long_blocks: 64, the threshold with the lowest
 * storm median in tools/parts_route_bench.py's sweep (profiles/parts_routed/README.md).
 * max_long: 16 x the device's compute units. long_bytes: 32 MiB, seven times the 4.76 MB
 * of that benchmark's pool of 100 EpochChange lists, which its storm names too. When no
 * list is long the call is the planned one plus two launches that find nothing to do:
 * on 2^20 one-part lists the two calls differ by less than their spread (the same file).
 *
 * ORDER: the lanes that remain are in descending block-count class, as in
 * msha_hash_actions_device_planned.
 *
 * ONE STREAM, capturable: the kernels (init, mark, measure, scan, scatter, copy, chain,
 * hash, fill) all go on `stream` (NULL: the context's own); there is no memset, no
 * library stream and no host wait. The workspace -- the planned entry's arrays, five
 * words a slot and the flatten buffer -- is this entry's own allocation in the context,
 * so calls of this and of the planned entry on one context share no memory. It grows by
 * hipMalloc only while `stream` is NOT being captured, and growing waits for the
 * previous routed call; on a capturing stream with too small a workspace (or a context
 * that has made no device call yet) the call fails with MSHA_ERR_INVALID_ARG and says
 * to make one call of that size outside the capture first. Outside capture a call is
 * ordered after the previous routed call of the context through a library event. A
 * captured call holds the workspace's addresses, as a captured planned call does.
 *
 * MSHA_PARTS_TIMING and MSHA_PARTS_PLAN_WAVE_SUM apply as in the planned entry.
 */
#define MSHA_HAS_PARTS_ROUTED 1
typedef struct {
  uint32_t long_blocks;  /* a named, valid list of >= this many 64-byte blocks is LONG; 0: the default */
  uint32_t max_long;     /* at most this many lists are routed per call; 0: 16 x CUs; above 16 x CUs: INVALID_ARG */
  uint64_t long_bytes;   /* bytes of the context's flatten buffer; 0: the default; below 16 + MSHA_DEVICE_ARENA_SLACK
                            or above 2^48: INVALID_ARG */
} msha_route_opts;       /* NULL: all defaults */
#define MSHA_ROUTE_LONG_BLOCKS_DEFAULT 64u
#define MSHA_ROUTE_LONG_BYTES_DEFAULT (32ull << 20)
int msha_hash_actions_device_routed(msha_ctx* ctx, const uint8_t* d_arena,
                                    const uint64_t* d_part_off, const uint64_t* d_part_len,
                                    const uint64_t* d_list_part_begin, uint64_t n_lists,
                                    const uint32_t* d_action_list, uint64_t n_actions,
                                    const msha_route_opts* opts, uint8_t* d_out, void* stream);
/* Counters of msha_hash_actions_device_routed (msha_parts_stats, msha_parts_plan_stats
 * and msha_concat_stats are untouched by it; its chain launch counts in msha_stats as
 * every chain launch does: launches_coop and launches_chain8). */
typedef struct {
  uint64_t calls;             /* calls that enqueued their launches */
  uint64_t actions;           /* digests they produce */
  uint64_t lists;             /* lists they were given */
  uint64_t launches_plan;     /* init, mark, measure, scan and scatter launches */
  uint64_t launches_copy;     /* k_concat_copy launches: one a call */
  uint64_t launches_chain;    /* eight-lane chain launches: one a call */
  uint64_t launches_hash;     /* k_digest_parts_planned launches */
  uint64_t launches_fill;     /* k_parts_fill launches (calls with d_action_list) */
  uint64_t last_lanes;        /* the last call's lists hashed as lanes, ... */
  uint64_t last_blocks;       /* ... the 64-byte blocks compressed for those, ... */
  uint64_t last_routed;       /* ... its routed lists and ... */
  uint64_t last_routed_bytes; /* ... the bytes of the flatten buffer they were given; all read back, and */
  double last_kernel_ms;      /* the call's kernels timed by HIP events, only under MSHA_PARTS_TIMING=1
                                 (read at each call; the call then waits for its kernels; never while
                                 `stream` is being captured); otherwise these five are 0 */
} msha_parts_route_stats;
int msha_get_parts_route_stats(const msha_ctx* ctx, msha_parts_route_stats* out);
/* Diagnostic, synchronous, like msha_parts_plan_read_order: waits for the device, then
 * copies the last routed call's routed list ids (in no particular order) into
 * lists[0 .. min(cap, *n_routed)), their count into *n_routed and the bytes of the
 * flatten buffer they were given into *routed_bytes. lists may be NULL when cap is 0. */
int msha_parts_route_read(msha_ctx* ctx, uint32_t* lists, uint64_t cap, uint64_t* n_routed,
                          uint64_t* routed_bytes);
/* The same for the lanes that remained: the last routed call's lane order, as
 * msha_parts_plan_read_order gives the planned entry's. */
int msha_parts_route_read_order(msha_ctx* ctx, uint32_t* order, uint64_t cap, uint64_t* lanes);

/*
 * Device stream sets: long writes routed to the chain (ABI 10, additive:
 * MSHA_HAS_STREAMS_DEVICE_ROUTED tells a build that has it). In a device stream set one
 * stream is one lane, which is right for tens of thousands of streams taking a few
 * digests each. NodeState.ActiveHash (pkg/testengine/recorder.go:288-359) is the other
 * shape: one stream a node, a handful of streams, each taking every committed request
 * digest between two checkpoints -- thousands of blocks in a row on a handful of lanes.
 * This entry is msha_dstreams_write_device with the decision made on the GPU inside the
 * call: it finds the rows whose write compresses many blocks, flattens each behind its
 * stream's buffered bytes and runs them on the eight-lane chain (the kernel of
 * msha_absorb_chain_device), and writes the other rows as lanes.
 *
 * SAME RESULT, SAME ERRORS as msha_dstreams_write_device. Rows and the row contract (a
 * stream at most once a call; a repeat leaves that stream alone unspecified and touches
 * nothing outside the set), the READ CONTRACT, the host checks (null pointers,
 * d_arena's alignment, n_rows >= 2^32 - 1, d_row NULL with n_rows != n), bit 32 for a
 * row naming a stream >= n and bit 4 for a decreasing part range (either stream
 * untouched), empty parts and zero-part rows contributing nothing, n_rows == 0
 * launching nothing: all are that entry's. Also checked on the host: the bounds of
 * `opts` (msha_route_opts above, the same bounds). Routing is an optimisation: no input
 * makes a stream's state, buffer or length differ from that entry's, and nothing here
 * raises bit 16.
 *
 * WHAT IS ROUTED. A row is LONG when its stream is < n, its part range is valid and
 *   whole = floor((length[s] % 64 + the sum of its part lengths) / 64) >= long_blocks,
 * whole being the blocks the write compresses. A long row claims a slot, then room for
 * round16(length[s] % 64 + sum) bytes, by the rules of msha_hash_actions_device_routed
 * (CAPS NEVER FAIL A CALL, above): a row that gets no slot or no room stays a lane and
 * is as right as any; when every long row fits both caps exactly the long rows are
 * routed; of long rows of one total L = length[s] % 64 + sum exactly
 * min(n_long, max_long, floor((long_bytes - MSHA_DEVICE_ARENA_SLACK) / round16(L))) are.
 *
 * DEFAULTS (a zero field, or opts NULL): max_long 16 x compute units, long_bytes 32 MiB,
 * long_blocks MSHA_DSTREAMS_ROUTE_LONG_BLOCKS_DEFAULT = 64, the routed parts entry's
 * threshold. tools/dstream_bench.py's `long` measure sweeps it from 8 to 256
 * (profiles/streams_device/long.jsonl and README.md): where the long rows are far above
 * it the medians differ by less than their spreads, so 64 stays; a threshold so low that
 * most of many thousand short rows count as long is the one setting measured to lose,
 * by a wide margin. With no long row the call costs three launches that find nothing to
 * do and two more than write_device; the same files name that loss.
 *
 * SIX LAUNCHES, all on `stream` (NULL: the context's own), whatever the rows hold: init,
 * measure, copy, chain, tail, write. No memset, no library stream, no host wait; the
 * call captures into a HIP graph as a chain of kernel nodes (a replay appends again).
 * With no long row the copy, the chain and the tail find nothing to do. No kernel waits
 * on another workgroup.
 *
 * The workspace (a byte a row, 36 bytes a slot and the flatten buffer of long_bytes)
 * belongs to the set and is freed in destroy. Growth, the refusal on a capturing stream
 * and the event that orders a call after the set's previous routed call are those of
 * msha_dstreams_write_jobs_device; the two entries share no memory.
 *
 * MSHA_PARTS_TIMING and MSHA_PARTS_PLAN_WAVE_SUM apply as in the routed parts entry.
 */
#define MSHA_HAS_STREAMS_DEVICE_ROUTED 1
#define MSHA_DSTREAMS_ROUTE_LONG_BLOCKS_DEFAULT 64u
int msha_dstreams_write_routed_device(msha_dstreams* set, const uint8_t* d_arena,
                                      const uint64_t* d_part_off, const uint64_t* d_part_len,
                                      const uint64_t* d_row_part_begin, const uint32_t* d_row,
                                      uint64_t n_rows, const msha_route_opts* opts, void* stream);
/* Counters of msha_dstreams_write_routed_device (msha_dstreams_stats and
 * msha_dstreams_jobs_stats count none of its calls; its chain launch counts in msha_stats
 * as every chain launch does: launches_coop and launches_chain8). */
typedef struct {
  uint64_t calls;             /* calls that enqueued their launches */
  uint64_t rows;              /* rows of those calls */
  uint64_t launches_route;    /* init and measure: 2 a call */
  uint64_t launches_copy;     /* the flatten: one a call */
  uint64_t launches_chain;    /* the eight-lane absorb chain: one a call */
  uint64_t launches_tail;     /* the routed streams' tail rows and lengths: one a call */
  uint64_t launches_write;    /* Write's row body over the rows that stayed lanes: one a call */
  uint64_t last_routed;       /* the last call's routed rows and ... */
  uint64_t last_routed_bytes; /* ... the bytes of the flatten buffer they were given; both read back, and */
  double last_kernel_ms;      /* the call's kernels timed by HIP events, only under MSHA_PARTS_TIMING=1
                                 (read at each call; the call then waits for its kernels; never while
                                 `stream` is being captured); otherwise these three are 0 */
} msha_dstreams_route_stats;
int msha_dstreams_get_route_stats(const msha_dstreams* set, msha_dstreams_route_stats* out);
/* Diagnostic, synchronous, like msha_parts_route_read: waits for the device, then copies
 * the row indices (r, not the streams) the set's last routed call routed, in no
 * particular order, into rows[0 .. min(cap, *n_routed)), their count into *n_routed and
 * the bytes of the flatten buffer they were given into *routed_bytes. rows may be NULL
 * when cap is 0. Before any routed call both counts are 0. */
int msha_dstreams_route_read(msha_dstreams* set, uint32_t* rows, uint64_t cap, uint64_t* n_routed,
                             uint64_t* routed_bytes);

/*
 * Device stream sets: jobs in call order with the long streams routed to the chain
 * (ABI 10, additive: MSHA_HAS_STREAMS_DEVICE_JOBS_ROUTED tells a build that has it).
 * NodeState.ActiveHash (pkg/testengine/recorder.go:288-359) is one stream a node, and
 * Apply writes every committed request digest to its node's stream in commit order: a
 * device-resident caller holds JOBS IN CALL ORDER whose few streams repeat and end up
 * long. msha_dstreams_write_jobs_device takes that order and runs each stream as one
 * lane; msha_dstreams_write_routed_device gives a long stream eight lanes and wants the
 * CSR grouped by stream. This entry joins them inside one call: the jobs are grouped by
 * stream on the GPU as in the first, and the grouped streams are written as in the
 * second, the long ones on the eight-lane chain.
 *
 * SAME RESULT, SAME ERRORS as msha_dstreams_write_jobs_device over the same jobs,
 * whatever `opts` holds: state, buffer and length of every stream are bit for bit that
 * entry's. A stream may be named any number of times and its chunks append in job
 * order; empty chunks contribute nothing; a job whose stream is >= n is DROPPED (no
 * stream touched, its chunk not read, every other job exact) and msha_device_status()
 * reports bit 32 once. The arena rules and the host checks (null pointers, d_arena's
 * alignment, n_jobs >= 2^32 - 1) are that entry's; the bounds of `opts` are checked on
 * the host as in msha_dstreams_write_routed_device. n_jobs == 0 returns MSHA_OK and
 * launches nothing. Nothing here raises bit 4 or bit 16.
 *
 * WHAT IS ROUTED is the paragraph of msha_dstreams_write_routed_device with "row" read
 * as "stream" and "its parts" as "its valid jobs". A stream is LONG when
 *   floor((length[s] % 64 + the sum of its jobs' lengths) / 64) >= long_blocks;
 * a dropped job's length counts for no stream. The caps never fail a call: a long
 * stream that gets no slot or no room stays a lane and is as right as any; when every
 * long stream fits both caps exactly the long streams are routed; of long streams of
 * one total L exactly
 * min(n_long, max_long, floor((long_bytes - MSHA_DEVICE_ARENA_SLACK) / round16(L))) are.
 * DEFAULTS as there: long_blocks MSHA_DSTREAMS_ROUTE_LONG_BLOCKS_DEFAULT, max_long 16 x
 * compute units, long_bytes 32 MiB.
 *
 * 3 * passes + 8 LAUNCHES (passes = ceil(bit_width(n) / 8)), all on `stream` (NULL: the
 * context's own): the jobs entry's sort passes and its two CSR kernels, then the routed
 * write's six in its order (init, measure, copy, chain, tail, write) over the grouped
 * offsets, lengths and CSR, where row r is stream r and every stream is a row. No
 * memset, no library stream, no host wait, and no kernel waits on another workgroup;
 * the call captures into a HIP graph as a linear chain of kernel nodes, and a replay
 * appends again. The six launches cover all n streams however few of them the jobs
 * touch: O(n) lanes a call, most of which find no part.
 *
 * The workspace is this entry's own: the jobs entry's arrays, then the routed write's
 * over n rows with its flatten buffer of long_bytes. A jobs call, a routed call and a
 * call of this entry on one set share no memory. It belongs to the set and is freed in
 * destroy; growth (a quarter of the arrays to spare, nothing for the buffer), the
 * refusal on a capturing stream and the event that orders a call after the set's
 * previous call of this entry are those of msha_dstreams_write_jobs_device.
 *
 * MEASURED (tools/dstream_bench.py jobs_long; profiles/streams_device/jobs_long.jsonl
 * and README.md "Measurement 5"): see that file for what this entry gains on a few
 * long streams and what it costs on many short ones. A caller that knows its streams
 * are short calls msha_dstreams_write_jobs_device.
 *
 * MSHA_PARTS_TIMING and MSHA_PARTS_PLAN_WAVE_SUM apply as in the routed write.
 */
#define MSHA_HAS_STREAMS_DEVICE_JOBS_ROUTED 1
int msha_dstreams_write_jobs_routed_device(msha_dstreams* set, const uint8_t* d_arena,
                                           const uint32_t* d_job_stream, const uint64_t* d_job_off,
                                           const uint64_t* d_job_len, uint64_t n_jobs,
                                           const msha_route_opts* opts, void* stream);
/* Counters of msha_dstreams_write_jobs_routed_device (msha_dstreams_stats,
 * msha_dstreams_jobs_stats and msha_dstreams_route_stats count none of its calls; its
 * chain launch counts in msha_stats as every chain launch does: launches_coop and
 * launches_chain8). */
typedef struct {
  uint64_t calls;             /* calls that enqueued their launches */
  uint64_t jobs;              /* jobs of those calls */
  uint64_t launches_sort;     /* histogram, scan and scatter launches: 3 a pass */
  uint64_t launches_rows;     /* the two CSR kernels */
  uint64_t launches_route;    /* init and measure: 2 a call */
  uint64_t launches_copy;     /* the flatten: one a call */
  uint64_t launches_chain;    /* the eight-lane absorb chain: one a call */
  uint64_t launches_tail;     /* the routed streams' tail rows and lengths: one a call */
  uint64_t launches_write;    /* Write's row body over the streams that stayed lanes: one a call */
  uint64_t last_passes;       /* radix passes of the last call: ceil(bit_width(n) / 8) */
  uint64_t last_jobs;
  uint64_t last_routed;       /* the last call's routed streams and ... */
  uint64_t last_routed_bytes; /* ... the bytes of the flatten buffer they were given; both read back, and */
  double last_kernel_ms;      /* the call's kernels timed by HIP events, only under MSHA_PARTS_TIMING=1
                                 (read at each call; the call then waits for its kernels; never while
                                 `stream` is being captured); otherwise these three are 0 */
} msha_dstreams_jobs_route_stats;
int msha_dstreams_get_jobs_route_stats(const msha_dstreams* set, msha_dstreams_jobs_route_stats* out);
/* Diagnostic, synchronous (waits for the device), for the set's last call of this entry:
 * the job order as msha_dstreams_jobs_read_order gives it (order[p] is the job applied
 * p-th, argsort(min(stream, n), stable) exactly, up to order_cap entries; *n_jobs that
 * call's job count, *n_valid how many leading positions are valid jobs), and the routed
 * streams as msha_dstreams_route_read gives the routed rows (the stream ids, in no
 * particular order, into streams[0 .. min(streams_cap, *n_routed)), their count into
 * *n_routed, the bytes of the flatten buffer they were given into *routed_bytes). order
 * and streams may be NULL when their cap is 0. Before any such call every count is 0.
 * msha_dstreams_jobs_read_order and msha_dstreams_route_read keep meaning the last jobs
 * call and the last routed call: this entry touches neither. */
int msha_dstreams_jobs_route_read(msha_dstreams* set, uint32_t* order, uint64_t order_cap,
                                  uint64_t* n_jobs, uint64_t* n_valid, uint32_t* streams,
                                  uint64_t streams_cap, uint64_t* n_routed, uint64_t* routed_bytes);

/*
 * Digests verified on the GPU (ABI 10, additive: MSHA_HAS_VERIFY_DEVICE tells a build
 * that has it). What the state machine does with almost every digest it gets back is
 * compare it with one it already holds: applyVerifyBatchHashResult compares a forwarded
 * batch's digest with VerifyBatch.ExpectedDigest (pkg/statemachine/batch_tracker.go:167-195),
 * a request's digest is compared with the digests other nodes acknowledged
 * (pkg/processor/clients.go:152-177), an EpochChange's with its acks
 * (epoch_target.go:486-528). This entry does that comparison where the device entries
 * above left the digests, so that a caller brings down 40 bytes (how many differ, which
 * is the first) and a short list instead of 32 bytes a digest. Measured times, against
 * the download and against the same expression in torch: profiles/verify/README.md.
 *
 * MATCH. Slot i, for i in [0, n), matches iff all 32 bytes of d_got[32 i ..] equal
 * d_expected[32 e ..], e = d_expected_idx ? d_expected_idx[i] : i. d_expected holds
 * n_expected rows; with d_expected_idx NULL slot i expects row i and n_expected must
 * equal n. An index may repeat (N nodes' acks of one request expect one row). An index
 * e >= n_expected is a mismatch: it counts in bad and in bad_index, and no byte of
 * d_expected is read for that slot. No bit of the device error word is used and
 * msha_device_status() is untouched by this entry: d_result carries everything.
 *
 * MASK. Bit i % 64 of d_bad_mask[i / 64] is 1 iff slot i differs. Every one of the
 * ceil(n / 64) words is written, and the bits at and past n in the last word are 0: the
 * caller never clears the mask.
 *
 * LIST. d_bad_list[0 .. listed) holds the first listed = min(bad, list_cap) differing
 * slots in ascending order. Entries at and past listed are not written. d_bad_list may
 * be NULL when list_cap is 0.
 *
 * RESULT. *d_result (device memory) is written whole by every call that launches.
 *
 * READ AND WRITE CONTRACT. Read: the 32 n bytes of d_got; of d_expected only rows that
 * some slot's index names, all below n_expected; the n entries of d_expected_idx (the
 * entries of differing slots twice). Written: the ceil(n / 64) mask words, the first
 * listed entries of d_bad_list, *d_result. Nothing else. d_bad_mask and d_result are
 * 8-byte aligned and d_bad_list and d_expected_idx 4-byte aligned, as their types say;
 * the outputs must not overlap the inputs.
 *
 * Checked on the host (MSHA_ERR_INVALID_ARG, each with a text): null pointers; d_got or
 * d_expected not MSHA_DEVICE_ALIGN-aligned; n at or above 2^32 - 1; n != n_expected
 * without d_expected_idx; list_cap > 0 with d_bad_list NULL. n == 0 returns MSHA_OK and
 * launches nothing (*d_result is left as it was).
 *
 * ONE STREAM, capturable: two kernels (compare, scan) go on `stream` (NULL: the
 * context's own). There is no memset, no library stream, no host wait and no workspace
 * of the context's, and no workgroup waits on another, so the call captures into a HIP
 * graph as two kernel nodes and a replay verifies what the arrays hold by then. The scan
 * is one workgroup, serial in chunks of msha_verify_stats.scan_words mask words; its
 * share of the call is in profiles/verify/README.md. The one allocation is the context's
 * error word on its first device call: on a capturing stream a context that has made no
 * device call yet fails with MSHA_ERR_INVALID_ARG and says to make one call of this size
 * outside the capture first.
 */
#define MSHA_HAS_VERIFY_DEVICE 1
typedef struct {
  uint64_t n;          /* digests compared */
  uint64_t bad;        /* slots that differ (out-of-range expected indices included) */
  uint64_t first_bad;  /* the smallest differing slot; n when bad == 0 */
  uint64_t listed;     /* min(bad, list_cap): entries written to d_bad_list */
  uint64_t bad_index;  /* of bad, slots whose d_expected_idx entry was >= n_expected */
} msha_verify_result;  /* device memory, written whole by every call */
int msha_verify_digests_device(msha_ctx* ctx,
                               const uint8_t* d_got, uint64_t n,
                               const uint8_t* d_expected, uint64_t n_expected,
                               const uint32_t* d_expected_idx,
                               uint64_t* d_bad_mask,
                               uint32_t* d_bad_list, uint64_t list_cap,
                               msha_verify_result* d_result, void* stream);
/* Counters of msha_verify_digests_device (msha_stats, msha_parts_stats and
 * msha_concat_stats are untouched by it). */
typedef struct {
  uint64_t calls;         /* calls that enqueued their launches */
  uint64_t digests;       /* slots they compared (n) */
  uint64_t launches;      /* kernel launches: two a call */
  uint64_t scan_words;    /* mask words the scan takes a chunk: a constant, valid from context creation */
  double last_kernel_ms;  /* the last call's kernels timed by HIP events, only under MSHA_PARTS_TIMING=1
                             (read at each call; the call then waits for its kernels; never while
                             `stream` is being captured); otherwise 0 */
} msha_verify_stats;
int msha_get_verify_stats(const msha_ctx* ctx, msha_verify_stats* out);

/*
 * Digests grouped by value on the GPU (ABI 10, additive: MSHA_HAS_GROUP_DEVICE tells a
 * build that has it). Beside comparing a digest with one it holds (the entry above), the
 * state machine uses almost every digest it receives as a MAP KEY: a sequence tallies how
 * many nodes sent the same digest (pkg/statemachine/sequence.go:73-74, 271-277, 331-340:
 * prepares and commits are map[string]int, agreements := s.prepares[string(s.digest)]),
 * a checkpoint's quorum is values map[string][]nodeID (checkpoints.go:264-290), the
 * request acks are keyed by string(ack.Digest) per (client, reqNo)
 * (client_hash_disseminator.go:346-349, 415-504), and so are batchesByDigest
 * (batch_tracker.go:20, 85-91) and parsedByDigest (epoch_change.go:23, 42-50). This entry
 * is that map for digests that lie in device memory: which of them are equal, how many of
 * each, and which value has the most, left in HBM in order of first occurrence. Its
 * d_group_first and d_group also are the table of distinct digests and the index into it
 * that msha_digest_of_digests_device and msha_verify_digests_device take. Measured times,
 * against the download with a host map and against a sort of the rows in torch, and where
 * it loses: profiles/group/README.md.
 *
 * KEY. Slot i's key, for i in [0, n), is (d_scope ? d_scope[i] : 0, the 32 bytes at
 * d_digests + 32 i). Two slots are in one group iff their keys are equal in all 36 bytes.
 * Equality is always that full compare: a hash or a tag that matches never joins two
 * slots by itself (a wrong join is a wrong quorum). d_scope is what lets one call serve
 * many maps: the sequence number, the checkpoint, the (client, reqNo) index.
 *
 * FIRST. d_first[i] is the smallest slot with slot i's key: the group's leader, <= i.
 *
 * GROUP. Groups are numbered 0 .. groups - 1 in ascending order of their leader, that is
 * in order of first occurrence. d_group[i] is the number of slot i's group, and
 * d_members[i] (d_members may be NULL) the number of slots in it.
 *
 * LIST. For g < listed = min(groups, group_cap), d_group_first[g] is group g's leader and
 * d_group_count[g] its member count. Entries at and past listed are not written. Both may
 * be NULL when group_cap is 0.
 *
 * RESULT. *d_result (device memory) is written whole by every call that launches.
 *
 * CANONICAL. Every output is a function of the inputs alone. The groups are found with an
 * open-addressing table of capacity bit_ceil(2 n) (at least 64) and a keyed hash, but no
 * output depends on the table's size, the hash, its seed or the order in which workgroups
 * ran: the same inputs give the same bytes in every call. The seed is 64 bits the context
 * draws when it is created (the digests come off the wire: with a fixed function a
 * sender could aim every key at one probe chain), and it changes time only.
 *
 * READ AND WRITE CONTRACT. Read: the 32 n bytes of d_digests, as whole 16-byte pieces (a
 * row may be read several times), and the n entries of d_scope. Written: d_first, d_group
 * and d_members, n entries each, the first listed entries of d_group_first and
 * d_group_count, and *d_result. Nothing else of the caller's is touched. d_first is
 * written by one kernel and read by later ones. d_result is 8-byte aligned and the
 * 32-bit arrays 4-byte aligned, as their types say; the outputs must not overlap the
 * inputs or one another.
 *
 * Checked on the host (MSHA_ERR_INVALID_ARG, each with a text): null pointers; d_digests
 * not MSHA_DEVICE_ALIGN-aligned; n above 2^30 (the table has at most 2^31 positions and a
 * position is a uint32_t); group_cap > 0 with d_group_first or d_group_count NULL. n == 0
 * returns MSHA_OK and launches nothing (*d_result is left as it was). No bit of the
 * device error word is used and msha_device_status() is untouched by this entry.
 *
 * ONE STREAM, capturable: six kernels (init, insert, resolve, scan, rank, fill: group.hip)
 * go on `stream` (NULL: the context's own), counted in msha_group_stats.launches. There is
 * no memset, no library stream and no host wait, every dependency is a kernel boundary and
 * no workgroup waits on another, so the call captures into a HIP graph as a chain of six
 * kernel nodes, and a replay groups what the arrays hold by then.
 *
 * WORKSPACE. The table, where each slot's probe stopped, the leaders' counts and ids and
 * the tile totals are a workspace of this entry's own in the context: 4 bytes a table
 * position (8 to 16 a slot), 12 bytes a slot and 4 a 256 slots, 20 to 28 bytes a slot in
 * all. It follows the rule of the other device calls' workspaces: it grows only outside
 * stream capture and never shrinks, a call outside capture is ordered after the previous
 * group call, whatever stream that was on, by an event, and on a capturing stream a call
 * that would have to allocate (the workspace, or a fresh context's error word) fails with
 * MSHA_ERR_INVALID_ARG and says to make one call of this size outside the capture first.
 * msha_ctx_destroy releases it.
 *
 * Two diagnostics, read at each call: MSHA_GROUP_SEED replaces the context's seed, and
 * MSHA_GROUP_FORCE_HOME=h gives every key the home position h mod capacity, so that a
 * test reaches the probe chain and its wrap-around at small shapes. Neither changes an
 * output byte.
 */
#define MSHA_HAS_GROUP_DEVICE 1
typedef struct {
  uint64_t n;          /* slots grouped */
  uint64_t groups;     /* distinct (scope, digest) keys */
  uint64_t listed;     /* min(groups, group_cap): entries written to d_group_first / d_group_count */
  uint64_t max_count;  /* members of the largest group */
  uint64_t max_group;  /* the smallest group id that has max_count members */
} msha_group_result;   /* device memory, written whole by every call that launches */
int msha_group_digests_device(msha_ctx* ctx,
                              const uint8_t* d_digests, uint64_t n,
                              const uint32_t* d_scope,        /* may be NULL */
                              uint32_t* d_first, uint32_t* d_group,
                              uint32_t* d_members,            /* may be NULL */
                              uint32_t* d_group_first, uint32_t* d_group_count, uint64_t group_cap,
                              msha_group_result* d_result, void* stream);
/* Counters of msha_group_digests_device (no other entry's counters move with it). */
typedef struct {
  uint64_t calls;         /* calls that enqueued their launches */
  uint64_t digests;       /* slots they grouped (n) */
  uint64_t launches;      /* kernel launches: six a call */
  uint64_t table_slots;   /* table positions of the last call: bit_ceil(2 n), at least 64 */
  double last_kernel_ms;  /* the last call's kernels timed by HIP events, only under MSHA_PARTS_TIMING=1
                             (read at each call; the call then waits for its kernels; never while
                             `stream` is being captured); otherwise 0 */
} msha_group_stats;
int msha_get_group_stats(const msha_ctx* ctx, msha_group_stats* out);

/*
 * Device digest maps (ABI 10, additive: MSHA_HAS_DIGEST_MAP tells a build that has them).
 * msha_group_digests_device answers for the n slots of one call and keeps nothing. The
 * maps it stands for fill up message by message, over many ActionLists: a sequence's
 * prepares and commits (pkg/statemachine/sequence.go:73-74, 271-277, 331-340), a
 * checkpoint's values (checkpoints.go:264-290), the request acks per (client, reqNo)
 * (client_hash_disseminator.go:346-349, 415-504); and what the state machine acts on is
 * the moment a key's count crosses a quorum (agreements := s.prepares[string(s.digest)]
 * against someCorrectQuorum / intersectionQuorum). A device digest map is that map kept in
 * HBM across calls: stable entry ids, running counts, and a per-call report of the keys
 * whose count crossed a threshold. Measured times, against regrouping everything seen so
 * far and against the download with a host map, and where it loses:
 * profiles/dmap/README.md.
 *
 * THE OBJECT. msha_dmap_create allocates, on the context's first device, everything the
 * map will ever hold, for max_keys in [1, 2^30] keys: the key store (uint32 scope[max_keys]
 * and 32-byte digest rows, 16-byte aligned) and uint32 count[max_keys], both indexed by
 * entry id; an open-addressing table uint32[capacity], capacity = bit_ceil(2 max_keys) and
 * at least 64, holding EMPTY or an id; and a small head of 64-bit words (`entries`, and
 * the words the kernels hand to one another): 4 bytes of scope, 32 of digest and 4 of
 * count a key, 40, plus 4 a table position, 8 to 16 a key: 48 to 56 bytes a key in all
 * (48 * 2^20 bytes and the head at max_keys = 2^20). Each of the five arrays is rounded up
 * to 256 bytes and the table has at least 64 positions, so a map of a few keys is about
 * 1.3 KiB whatever max_keys says. A map is destroyed before its context, and every call on
 * it takes the context's lock. The seed of its keyed hash is 64 bits drawn at create, for the
 * reason given under CANONICAL of the entry above.
 *
 * An ENTRY ID is a key's position in order of first occurrence over the map's whole life
 * since the last clear. It never changes. There is no erase (open addressing would need
 * tombstones): a caller drops a whole map, a checkpoint window, with msha_dmap_clear_device.
 * Multi-GPU maps are out of scope as well. In a map made by msha_dmap_create a slot is a
 * vote, and the caller hands each vote in once; a map that counts each sender once a key
 * is the vote map of "Device digest maps that count voters" below.
 *
 * msha_dmap_add_device.
 *
 * KEY. As in msha_group_digests_device: slot i's key is (d_scope ? d_scope[i] : 0, the 32
 * bytes at d_digests + 32 i). Equality is the full 36-byte compare, always: between the
 * slots of the call, and against the stored keys.
 *
 * ID. d_id[i] is the entry id of slot i's key. Keys already in the map keep their id. Keys
 * new in this call get entries_before + r, r their rank by first occurrence in this call
 * AMONG THE NEW KEYS: existing keys that lie between two new ones use up no number.
 *
 * COUNTS. d_before[i] is the key's count before the call, 0 for a new key; d_after[i] is
 * d_before[i] plus the slots of this call that hold the key, and becomes the key's count.
 * The count saturates at 2^32 - 1. Both arrays may be NULL.
 *
 * CROSSED. A key crossed when threshold > 0 && before < threshold && threshold <= after.
 * d_crossed_slot[0 .. listed) holds the call's leader slot of each crossing key, the key's
 * smallest slot in this call, in ascending order; listed = min(crossed, crossed_cap).
 * Entries at and past listed are not written. d_crossed_slot may be NULL with crossed_cap
 * 0. From a leader slot the caller has d_id, d_scope and the digest in its own arrays.
 *
 * FULL: ALL OR NOTHING. The call is refused whole if entries_before + added > max_keys
 * (added: the new keys of this call). result.full is then 1 and every d_id[i] is
 * 0xFFFFFFFF; d_before and d_after are still written as described, for inspection (new
 * keys have before 0); crossed is 0 and nothing is listed; and no byte of the map changes:
 * not the table, the keys, the counts or entries. A call that fits exactly succeeds.
 *
 * RESULT. *d_result (device memory) is written whole by every call that launches. When
 * full, max_count and max_id are 0.
 *
 * CANONICAL. Every output, and every byte msha_dmap_read returns, is a function of the
 * sequence of calls alone: none depends on the seed, on where a key landed in the table,
 * or on the order workgroups ran in.
 *
 * READ AND WRITE CONTRACT. Read: the 32 n bytes of d_digests, as whole 16-byte pieces (a
 * row may be read several times), and the n entries of d_scope. Written: d_id and the two
 * optional arrays, n entries each, the first listed entries of d_crossed_slot, and
 * *d_result. Nothing else of the caller's is touched. d_result is 8-byte aligned and the
 * 32-bit arrays 4-byte aligned, as their types say; the outputs must not overlap the
 * inputs or one another.
 *
 * Checked on the host (MSHA_ERR_INVALID_ARG, each with a text): null pointers; d_digests
 * not MSHA_DEVICE_ALIGN-aligned; n above 2^30; crossed_cap > 0 with d_crossed_slot NULL.
 * n == 0 returns MSHA_OK and launches nothing (*d_result is left as it was). No bit of the
 * device error word is used and msha_device_status() is untouched by a map.
 *
 * ONE STREAM, capturable: seven kernels go on `stream` (NULL: the context's own), counted
 * in msha_dmap_stats.launches: the init, insert and resolve of msha_group_digests_device,
 * on a table of the call's own, find the call's leaders; then find (leaders look their
 * key up in the map, read-only), scan (one workgroup: the numbers and the decision),
 * commit (nothing when full) and fill (dmap.hip). There is no memset, no library stream
 * and no host wait, every dependency is a kernel boundary and no workgroup waits on
 * another, so the call captures into a HIP graph as a linear chain of seven kernel nodes,
 * and a replay adds again.
 *
 * WORKSPACE. The call's table and per-slot scratch are a workspace the map owns (the
 * group entry's workspace and counters are untouched by a map call): 4 bytes a position of
 * the call's table (8 to 16 a slot), 24 bytes a slot and 12 a 256 slots. It follows the
 * rule of the other device calls' workspaces: it grows only outside stream capture and
 * never shrinks, a call outside capture is ordered after the map's previous add, whatever
 * stream that was on, by an event, and on a capturing stream a call that would have to
 * allocate fails with MSHA_ERR_INVALID_ARG and says to make one call of this size outside
 * the capture first; the map is unchanged then. Ordering against finds and clears on other
 * HIP streams is the caller's.
 *
 * msha_dmap_find_device: one kernel, a lane a slot, read-only. d_id[i] and d_count[i]
 * (d_count may be NULL) are the id and the count of slot i's key, or 0xFFFFFFFF and 0 if
 * the map does not hold it. It changes nothing and captures as one kernel node. Host
 * checks as for add. msha_dmap_clear_device: one kernel; the table goes to EMPTY and
 * entries to 0 (counts and keys need no clearing: new ids overwrite them).
 *
 * msha_dmap_size and msha_dmap_read take host memory and wait for the device, as
 * msha_dstreams_length and _export do. read copies entries first_id .. first_id + k: k
 * scopes, 32 k digest bytes and k counts (each array may be NULL); a range that reaches
 * past entries is MSHA_ERR_INVALID_ARG.
 *
 * Two diagnostics, read at each call: MSHA_DMAP_SEED replaces the map's seed, and
 * MSHA_DMAP_FORCE_HOME=h gives every key the home position h mod capacity in the map's
 * table, so that a test reaches the probe chain and its wrap-around at small shapes. A key
 * is looked for where the values in force would have put it, so each keeps one value from
 * a clear (or create) to the next; then neither changes an output byte. MSHA_GROUP_SEED
 * and MSHA_GROUP_FORCE_HOME keep acting on the call's table.
 */
#define MSHA_HAS_DIGEST_MAP 1
typedef struct msha_dmap msha_dmap;
typedef struct {
  uint64_t n;          /* slots added */
  uint64_t entries;    /* keys in the map after the call */
  uint64_t added;      /* keys of this call the map did not hold */
  uint64_t full;       /* 1: the call was refused whole, the map is as it was */
  uint64_t crossed;    /* keys whose count crossed the threshold in this call */
  uint64_t listed;     /* min(crossed, crossed_cap): entries written to d_crossed_slot */
  uint64_t max_count;  /* the largest count after the call among the keys it touched */
  uint64_t max_id;     /* the smallest entry id that has it */
} msha_dmap_result;    /* device memory, written whole by every call that launches */
int msha_dmap_create(msha_ctx* ctx, uint64_t max_keys, msha_dmap** out);
void msha_dmap_destroy(msha_dmap* map);
int msha_dmap_add_device(msha_dmap* map,
                         const uint8_t* d_digests, uint64_t n,
                         const uint32_t* d_scope,            /* may be NULL */
                         uint32_t threshold,
                         uint32_t* d_id,
                         uint32_t* d_before, uint32_t* d_after,  /* each may be NULL */
                         uint32_t* d_crossed_slot, uint64_t crossed_cap,
                         msha_dmap_result* d_result, void* stream);
int msha_dmap_find_device(msha_dmap* map,
                          const uint8_t* d_digests, uint64_t n,
                          const uint32_t* d_scope,           /* may be NULL */
                          uint32_t* d_id,
                          uint32_t* d_count,                 /* may be NULL */
                          void* stream);
int msha_dmap_clear_device(msha_dmap* map, void* stream);
int msha_dmap_size(msha_dmap* map, uint64_t* entries);
int msha_dmap_read(msha_dmap* map, uint64_t first_id, uint64_t k,
                   uint32_t* scope_out, uint8_t* digests_out, uint32_t* count_out);
/* Counters of one map (no other entry's counters move with it). */
typedef struct {
  uint64_t adds;          /* add calls that enqueued their launches */
  uint64_t finds;         /* find calls */
  uint64_t clears;        /* clear calls (the one inside create is not counted) */
  uint64_t digests;       /* slots of the adds and finds (n) */
  uint64_t launches;      /* kernel launches: seven an add, one a find, one a clear */
  uint64_t capacity;      /* table positions: bit_ceil(2 max_keys), at least 64 */
  double last_kernel_ms;  /* the last call's kernels timed by HIP events, only under MSHA_PARTS_TIMING=1
                             (read at each call; the call then waits for its kernels; never while
                             `stream` is being captured); otherwise 0 */
} msha_dmap_stats;
int msha_dmap_get_stats(const msha_dmap* map, msha_dmap_stats* out);

/*
 * Device digest maps that count voters (ABI 10, additive: MSHA_HAS_DIGEST_VOTE_MAP tells a
 * build that has them). A map made by msha_dmap_create counts slots. Two of the maps it
 * stands for count NODES: the request acks are a set, cr.agreements[source] = struct{}{},
 * every quorum test is len(cr.agreements) (client_hash_disseminator.go:814-832, 492-500),
 * the set is asked "has node X acked" (:296, :395, sequence.go:218) and listed as node ids
 * (:647-649); a checkpoint's values are map[string][]nodeID (checkpoints.go:264-280),
 * compared with the node's own id (:284). A replica that sends the same ack twice -- a
 * retransmission, a Byzantine sender, our own ack arriving after we stored the request --
 * must not move a key towards someCorrectQuorum. A VOTE MAP is a device digest map whose
 * count for a key is the number of distinct voters that voted for it, the set of voters
 * kept in HBM beside the key, so that no caller has to download digests to deduplicate
 * (key, sender) on the host. Measured times, against msha_dmap_add_device over the same
 * slots and against the download with a host dict of sets: profiles/dmap_vote/README.md.
 *
 * THE OBJECT. msha_dmap_create_voters(ctx, max_keys, max_voters, &map): max_keys as for
 * msha_dmap_create, max_voters in [1, 1024]. The map owns everything a plain map owns, in
 * the same layout, and behind it a voter mask per entry id: uint32 mask[max_keys][words],
 * words = ceil(max_voters / 32); bit v % 32 of word v / 32 stands for voter v. The mask
 * store adds 4 words bytes a key to the 48 to 56 of a plain map (4 bytes a key up to 32
 * voters, 128 at 1024), rounded up to 256 bytes like the other arrays. A new key's mask is
 * empty. INVARIANT: count[id] == popcount(mask[id]) at every kernel boundary outside a
 * vote call. msha_dmap_add_device on a vote map is refused (MSHA_ERR_INVALID_ARG, with a
 * text): it would break the invariant; on a plain map the three vote entries below are
 * refused the same way. msha_dmap_find_device, _size, _read, _destroy and _get_stats work
 * on both kinds unchanged. msha_dmap_clear_device on a vote map empties the masks as well:
 * still one kernel, still one launch counted.
 *
 * msha_dmap_vote_device. KEY and ID exactly as in msha_dmap_add_device (first-occurrence
 * numbering among the new keys, ids stable). d_voter[i] (uint32) is slot i's sender.
 *
 * COUNTED. d_counted[i] (uint32, 0 or 1; may be NULL) is 1 iff (a) d_voter[i] < max_voters,
 * (b) no slot j < i of this call has slot i's key and slot i's voter, and (c) the key's
 * mask before the call has no bit for d_voter[i] (a new key has an empty mask). Of several
 * equal votes in one call the smallest slot is the one counted: a function of the inputs,
 * not of the order lanes ran in.
 *
 * COUNTS. d_before[i] is the key's count before the call; d_after[i] is d_before[i] plus
 * the counted slots of the key in this call, and becomes the key's count. Nothing
 * saturates: count <= max_voters. A key none of whose slots is counted is still entered
 * and keeps or gets its id; its count may be 0, if all its voters were out of range.
 *
 * CROSSED. threshold > 0 && before < threshold && threshold <= after on these counts;
 * d_crossed_slot[0 .. listed) holds the leader slots of the crossing keys in ascending
 * order, listed = min(crossed, crossed_cap), exactly as for add.
 *
 * FULL: ALL OR NOTHING, the rule of add: refused whole when entries_before + added >
 * max_keys. Every d_id[i] is then 0xFFFFFFFF; d_counted, d_before and d_after are still
 * written as defined above, read-only facts about the map as it was; crossed is 0 and
 * nothing is listed; and no byte of the map changes: not the table, the keys, the counts,
 * the masks or entries.
 *
 * RESULT. msha_dmap_vote_result is eleven uint64_t: add's eight fields in add's order, then
 * counted (slots with d_counted 1), repeats (slots with a voter in range that were not
 * counted) and bad_voters (slots with d_voter[i] >= max_voters: a caller's error made
 * visible; no bit of the device error word is used and msha_device_status() is untouched).
 * When full, counted, repeats and bad_voters are still reported; max_count and max_id are
 * 0 as for add.
 *
 * CANONICAL. Every output, and every byte msha_dmap_read and msha_dmap_read_voters return,
 * is a function of the sequence of calls alone.
 *
 * Checked on the host as for add, and: d_voter NULL; a plain map. n == 0 returns MSHA_OK
 * before any other check and launches nothing. Read in addition to add's: the n entries of
 * d_voter. Written in addition: the n entries of d_counted.
 *
 * ONE STREAM, capturable, a linear chain: TEN kernels go on `stream` (NULL: the context's
 * own), counted in msha_dmap_vote_stats.launches: the init, insert and resolve of
 * msha_group_digests_device on the call's own table; find (leaders look their key up,
 * read-only; the same launch empties the call's pair table); pair (a second table of the
 * call's joins equal (key, voter) pairs, an entry the smallest slot of its pair); count
 * (the pair leaders whose bit the key's mask lacks are the counted slots; each key's are
 * summed); totals; scan (one workgroup: the numbers and the decision); commit (nothing
 * when full; ids, keys, counts, the crossed list); and fill (the outputs; unless full, each
 * counted slot sets its bit with a 32-bit atomic OR, a launch behind commit so that a new
 * id is there first). No memset, no library stream, no host wait, every dependency a
 * kernel boundary, no workgroup waits on another: the call captures into a HIP graph as a
 * linear chain of ten kernel nodes, and a replay votes again (and counts nothing new).
 * The workspace (the add's, then 4 bytes a position of the pair table, 8 to 16 a slot, 12
 * bytes a slot and 12 a 256 slots) follows add's rule; a capture that would have to
 * allocate is refused with the text naming msha_dmap_vote_device, the map unchanged.
 *
 * msha_dmap_find_votes_device: one kernel, read-only: find's answers (d_count may be NULL)
 * plus d_voted[i] = 1 iff the key is held and d_voter[i]'s bit is set; absent keys and
 * voters out of range give 0: _, ok := cr.agreements[nodeID(id)].
 * msha_dmap_read_voters: a host read like msha_dmap_read: the k * words mask words of
 * entries first_id .. first_id + k, with read's range check and message.
 * msha_dmap_get_vote_stats: vote calls move only this struct; msha_dmap_stats keeps its
 * layout and its adds, finds and launches do not move with them. A clear counts where it
 * does on a plain map.
 *
 * Diagnostics, read at each call: MSHA_DMAP_SEED and MSHA_DMAP_FORCE_HOME keep their
 * meaning; MSHA_DMAP_PAIR_FORCE_HOME=h gives every (key, voter) pair the home position h
 * mod capacity in the call's pair table (capacity bit_ceil(2 n), at least 64). None of
 * them changes an output byte.
 *
 * Out of scope: erase (as above); multi-GPU maps; more than 1024 voters; the Go adapter
 * and include/mirbft/processor.hpp; any change to msha_dmap_add_device.
 */
#define MSHA_HAS_DIGEST_VOTE_MAP 1
typedef struct {
  uint64_t n, entries, added, full, crossed, listed, max_count, max_id; /* as msha_dmap_result */
  uint64_t counted;     /* slots with d_counted 1 */
  uint64_t repeats;     /* slots with a voter in range that were not counted */
  uint64_t bad_voters;  /* slots with d_voter[i] >= max_voters */
} msha_dmap_vote_result; /* device memory, written whole by every call that launches */
int msha_dmap_create_voters(msha_ctx* ctx, uint64_t max_keys, uint32_t max_voters, msha_dmap** out);
int msha_dmap_vote_device(msha_dmap* map,
                          const uint8_t* d_digests, uint64_t n,
                          const uint32_t* d_scope,           /* may be NULL */
                          const uint32_t* d_voter,
                          uint32_t threshold,
                          uint32_t* d_id,
                          uint32_t* d_counted,               /* may be NULL */
                          uint32_t* d_before, uint32_t* d_after,  /* each may be NULL */
                          uint32_t* d_crossed_slot, uint64_t crossed_cap,
                          msha_dmap_vote_result* d_result, void* stream);
int msha_dmap_find_votes_device(msha_dmap* map,
                                const uint8_t* d_digests, uint64_t n,
                                const uint32_t* d_scope,     /* may be NULL */
                                const uint32_t* d_voter,
                                uint32_t* d_id,
                                uint32_t* d_count,           /* may be NULL */
                                uint32_t* d_voted,
                                void* stream);
int msha_dmap_read_voters(msha_dmap* map, uint64_t first_id, uint64_t k, uint32_t* masks_out);
/* Counters of one vote map's vote calls (no other counters move with them). */
typedef struct {
  uint64_t votes;         /* vote calls that enqueued their launches */
  uint64_t vote_finds;    /* find_votes calls */
  uint64_t slots;         /* slots of the votes and find_votes (n) */
  uint64_t launches;      /* kernel launches: ten a vote, one a find_votes */
  uint64_t max_voters;    /* as created; 0 on a plain map */
  uint64_t mask_words;    /* ceil(max_voters / 32) */
  double last_kernel_ms;  /* as in msha_dmap_stats: only under MSHA_PARTS_TIMING=1 */
} msha_dmap_vote_stats;
int msha_dmap_get_vote_stats(const msha_dmap* map, msha_dmap_vote_stats* out);

/*
 * Host-only helpers (no GPU needed).
 * msha_blocks_for_len: number of 64-byte compressions for an L-byte message,
 *   floor(L/64) + (L%64 < 56 ? 1 : 2)  (FIPS 180-4 5.1.1 padding).
 * msha_partition_by_blocks: split messages [0, n) into n_shards contiguous
 *   ranges of near-equal cumulative block count; bounds[0..n_shards]
 *   (bounds[0] = 0, bounds[n_shards] = n). Used for multi-GPU sharding.
 */
uint64_t msha_blocks_for_len(uint64_t len);
/* Permutation of [0, n) ordering messages by descending block count (stable). */
int msha_order_by_blocks(const uint64_t* len, uint64_t n, uint32_t* order);
int msha_partition_by_blocks(const uint64_t* len, uint64_t n, uint32_t n_shards,
                             uint64_t* bounds);
/* Alias detection the host entry points run before hashing (EpochChange
 * payloads re-hashed N^2 times, epoch_target.go:486-505): first[i] = the
 * smallest j <= i with (off[j], len[j]) == (off[i], len[i]); such messages are
 * hashed once and share the digest. */
int msha_alias_first(const uint64_t* off, const uint64_t* len, uint64_t n, uint64_t* first);

#ifdef __cplusplus
}
#endif

#endif /* MIRSHA_H_ */
