"""ctypes binding of libmirsha.so (the C ABI in include/mirsha.h).

The library is built in-tree (``mirbft_amd/libmirsha.so``, see
``mirbft_amd/csrc/Makefile`` and ``__graft_entry__.build()``). Loading fails
loudly when it is missing: there is no Python or CPU fallback for hashing.
"""
from __future__ import annotations

import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCT_LIB_PATH = os.path.join(_HERE, "libmirsha.so")
# MSHA_LIB_PATH loads a diagnostic or A/B variant built OUTSIDE the package
# (mirbft_amd/csrc/Makefile: BUILD=... OUT=...), so no experiment ever writes
# over the product library. Such a build is not the tree's: GPU test sessions
# and bench.py refuse it unless MSHA_ALLOW_FOREIGN_LIB=1.
LIB_PATH = os.environ.get("MSHA_LIB_PATH") or PRODUCT_LIB_PATH
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mirsha.h")

ABI_VERSION = 10
MSHA_OK = 0
MSHA_ERR_INVALID_ARG = 1
MSHA_ERR_NO_DEVICE = 2
MSHA_ERR_HIP = 3
MSHA_ERR_OUT_OF_MEMORY = 4
MSHA_ERR_ALIGNMENT = 5
MSHA_DEVICE_ARENA_SLACK = 64
MSHA_DEVICE_ALIGN = 16
MSHA_KERNEL_AUTO = 0
MSHA_KERNEL_LANE = 1
MSHA_KERNEL_COOP = 2
MSHA_STREAM_STATE_BYTES = 108
MSHA_PARTS_FOLD = 1
MSHA_HAS_PLANNED_READ = 1
MSHA_HAS_PARTS_CONCAT = 1
MSHA_HAS_PARTS_ROUTED = 1
MSHA_HAS_VERIFY_DEVICE = 1
MSHA_HAS_GROUP_DEVICE = 1
MSHA_HAS_DIGEST_MAP = 1
MSHA_HAS_DIGEST_VOTE_MAP = 1
MSHA_ROUTE_LONG_BLOCKS_DEFAULT = 64
MSHA_ROUTE_LONG_BYTES_DEFAULT = 32 << 20
MSHA_HAS_STREAMS_DEVICE = 1
MSHA_HAS_STREAMS_DEVICE_JOBS = 1
MSHA_HAS_ABSORB_CHAIN = 1
MSHA_HAS_STREAMS_DEVICE_ROUTED = 1
MSHA_DSTREAMS_ROUTE_LONG_BLOCKS_DEFAULT = 64
MSHA_HAS_STREAMS_DEVICE_JOBS_ROUTED = 1

_u8p = ctypes.POINTER(ctypes.c_uint8)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_ctxp = ctypes.c_void_p


class MshaStats(ctypes.Structure):
    _fields_ = [
        ("calls", ctypes.c_uint64),
        ("messages", ctypes.c_uint64),
        ("message_bytes", ctypes.c_uint64),
        ("blocks", ctypes.c_uint64),
        ("plan_ms", ctypes.c_double),
        ("pack_ms", ctypes.c_double),
        ("device_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
        ("direct_calls", ctypes.c_uint64),
        ("launches_lane", ctypes.c_uint64),
        ("launches_pipe", ctypes.c_uint64),
        ("launches_coop", ctypes.c_uint64),
        ("launches_split", ctypes.c_uint64),
        ("launches_dod", ctypes.c_uint64),
        ("split_retries", ctypes.c_uint64),
        ("h2d_bytes", ctypes.c_uint64),
        ("d2h_bytes", ctypes.c_uint64),
        ("small_calls", ctypes.c_uint64),
        ("staged_calls", ctypes.c_uint64),
        ("planned_device_calls", ctypes.c_uint64),
        ("launches_chain2", ctypes.c_uint64),
        ("launches_chain8", ctypes.c_uint64),
        ("small_zc_calls", ctypes.c_uint64),
        ("launches_lane_ws", ctypes.c_uint64),
    ]


class MshaShardStats(ctypes.Structure):
    _fields_ = [
        ("device", ctypes.c_int32),
        ("head_lanes", ctypes.c_uint32),
        ("messages", ctypes.c_uint64),
        ("lanes", ctypes.c_uint64),
        ("h2d_payload_bytes", ctypes.c_uint64),
        ("h2d_bytes", ctypes.c_uint64),
        ("d2h_bytes", ctypes.c_uint64),
        ("launches", ctypes.c_uint64),
        ("gather_begin_ms", ctypes.c_double),
        ("gather_end_ms", ctypes.c_double),
        ("gather_ms", ctypes.c_double),
        ("device_ms", ctypes.c_double),
        ("upload_ms", ctypes.c_double),
        ("kernel_ms", ctypes.c_double),
        ("first_launch_ms", ctypes.c_double),
        ("plan_kernel_ms", ctypes.c_double),
    ]


class MshaClockInfo(ctypes.Structure):
    _fields_ = [
        ("ghz_median", ctypes.c_double),
        ("ghz_min", ctypes.c_double),
        ("ghz_max", ctypes.c_double),
        ("kernel_ms", ctypes.c_double),
        ("gblocks_per_s", ctypes.c_double),
        ("workgroups", ctypes.c_uint32),
        ("blocks_per_lane", ctypes.c_uint32),
    ]


class MshaStreamsStats(ctypes.Structure):
    _fields_ = [
        ("writes", ctypes.c_uint64),
        ("sums", ctypes.c_uint64),
        ("bytes_written", ctypes.c_uint64),
        ("blocks_absorbed", ctypes.c_uint64),
        ("blocks_finished", ctypes.c_uint64),
        ("launches_absorb", ctypes.c_uint64),
        ("launches_finish", ctypes.c_uint64),
        ("buffered_only_writes", ctypes.c_uint64),
        ("pieces", ctypes.c_uint64),
        ("last_load_mode", ctypes.c_uint32),
        ("last_lanes", ctypes.c_uint32),
        ("last_kernel_ms", ctypes.c_double),
    ]


class MshaPlannedPlan(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_uint64),
        ("folded", ctypes.c_uint32),
        ("lanes", ctypes.c_uint32),
        ("head", ctypes.c_uint32),
        ("early", ctypes.c_uint32),
        ("late", ctypes.c_uint32),
        ("long_lanes", ctypes.c_uint32),
        ("long_listed", ctypes.c_uint32),
        ("gate", ctypes.c_uint32),
        ("long_cap", ctypes.c_uint32),
        ("head_cap", ctypes.c_uint32),
        ("head_per_wg", ctypes.c_uint32),
        ("gave_up", ctypes.c_uint64),
    ]


class MshaPartsStats(ctypes.Structure):
    _fields_ = [
        ("calls", ctypes.c_uint64),
        ("actions", ctypes.c_uint64),
        ("launches", ctypes.c_uint64),
        ("last_lanes", ctypes.c_uint64),
        ("last_kernel_ms", ctypes.c_double),
    ]


class MshaPartsPlanStats(ctypes.Structure):
    _fields_ = [
        ("calls", ctypes.c_uint64),
        ("actions", ctypes.c_uint64),
        ("lists", ctypes.c_uint64),
        ("last_lanes", ctypes.c_uint64),
        ("last_blocks", ctypes.c_uint64),
        ("launches_plan", ctypes.c_uint64),
        ("launches_hash", ctypes.c_uint64),
        ("launches_fill", ctypes.c_uint64),
        ("last_kernel_ms", ctypes.c_double),
    ]


class MshaConcatStats(ctypes.Structure):
    _fields_ = [
        ("calls", ctypes.c_uint64),
        ("lists", ctypes.c_uint64),
        ("launches", ctypes.c_uint64),
        ("last_bytes", ctypes.c_uint64),
        ("last_kernel_ms", ctypes.c_double),
    ]


class MshaVerifyResult(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_uint64),
        ("bad", ctypes.c_uint64),
        ("first_bad", ctypes.c_uint64),
        ("listed", ctypes.c_uint64),
        ("bad_index", ctypes.c_uint64),
    ]


class MshaVerifyStats(ctypes.Structure):
    _fields_ = [
        ("calls", ctypes.c_uint64),
        ("digests", ctypes.c_uint64),
        ("launches", ctypes.c_uint64),
        ("scan_words", ctypes.c_uint64),
        ("last_kernel_ms", ctypes.c_double),
    ]


class MshaGroupResult(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_uint64),
        ("groups", ctypes.c_uint64),
        ("listed", ctypes.c_uint64),
        ("max_count", ctypes.c_uint64),
        ("max_group", ctypes.c_uint64),
    ]


class MshaGroupStats(ctypes.Structure):
    _fields_ = [
        ("calls", ctypes.c_uint64),
        ("digests", ctypes.c_uint64),
        ("launches", ctypes.c_uint64),
        ("table_slots", ctypes.c_uint64),
        ("last_kernel_ms", ctypes.c_double),
    ]


class MshaDmapResult(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_uint64),
        ("entries", ctypes.c_uint64),
        ("added", ctypes.c_uint64),
        ("full", ctypes.c_uint64),
        ("crossed", ctypes.c_uint64),
        ("listed", ctypes.c_uint64),
        ("max_count", ctypes.c_uint64),
        ("max_id", ctypes.c_uint64),
    ]


class MshaDmapStats(ctypes.Structure):
    _fields_ = [
        ("adds", ctypes.c_uint64),
        ("finds", ctypes.c_uint64),
        ("clears", ctypes.c_uint64),
        ("digests", ctypes.c_uint64),
        ("launches", ctypes.c_uint64),
        ("capacity", ctypes.c_uint64),
        ("last_kernel_ms", ctypes.c_double),
    ]


class MshaDmapVoteResult(ctypes.Structure):
    _fields_ = MshaDmapResult._fields_ + [
        ("counted", ctypes.c_uint64),
        ("repeats", ctypes.c_uint64),
        ("bad_voters", ctypes.c_uint64),
    ]


class MshaDmapVoteStats(ctypes.Structure):
    _fields_ = [
        ("votes", ctypes.c_uint64),
        ("vote_finds", ctypes.c_uint64),
        ("slots", ctypes.c_uint64),
        ("launches", ctypes.c_uint64),
        ("max_voters", ctypes.c_uint64),
        ("mask_words", ctypes.c_uint64),
        ("last_kernel_ms", ctypes.c_double),
    ]


class MshaRouteOpts(ctypes.Structure):
    _fields_ = [
        ("long_blocks", ctypes.c_uint32),
        ("max_long", ctypes.c_uint32),
        ("long_bytes", ctypes.c_uint64),
    ]


class MshaPartsRouteStats(ctypes.Structure):
    _fields_ = [
        ("calls", ctypes.c_uint64),
        ("actions", ctypes.c_uint64),
        ("lists", ctypes.c_uint64),
        ("launches_plan", ctypes.c_uint64),
        ("launches_copy", ctypes.c_uint64),
        ("launches_chain", ctypes.c_uint64),
        ("launches_hash", ctypes.c_uint64),
        ("launches_fill", ctypes.c_uint64),
        ("last_lanes", ctypes.c_uint64),
        ("last_blocks", ctypes.c_uint64),
        ("last_routed", ctypes.c_uint64),
        ("last_routed_bytes", ctypes.c_uint64),
        ("last_kernel_ms", ctypes.c_double),
    ]


class MshaDstreamsStats(ctypes.Structure):
    _fields_ = [
        ("writes", ctypes.c_uint64),
        ("sums", ctypes.c_uint64),
        ("snaps", ctypes.c_uint64),
        ("resets", ctypes.c_uint64),
        ("launches", ctypes.c_uint64),
        ("last_rows", ctypes.c_uint64),
        ("last_kernel_ms", ctypes.c_double),
    ]


class MshaDstreamsJobsStats(ctypes.Structure):
    _fields_ = [
        ("calls", ctypes.c_uint64),
        ("jobs", ctypes.c_uint64),
        ("launches_sort", ctypes.c_uint64),
        ("launches_rows", ctypes.c_uint64),
        ("launches_write", ctypes.c_uint64),
        ("last_passes", ctypes.c_uint64),
        ("last_jobs", ctypes.c_uint64),
        ("tile_jobs", ctypes.c_uint64),
        ("last_kernel_ms", ctypes.c_double),
    ]


class MshaDstreamsRouteStats(ctypes.Structure):
    _fields_ = [
        ("calls", ctypes.c_uint64),
        ("rows", ctypes.c_uint64),
        ("launches_route", ctypes.c_uint64),
        ("launches_copy", ctypes.c_uint64),
        ("launches_chain", ctypes.c_uint64),
        ("launches_tail", ctypes.c_uint64),
        ("launches_write", ctypes.c_uint64),
        ("last_routed", ctypes.c_uint64),
        ("last_routed_bytes", ctypes.c_uint64),
        ("last_kernel_ms", ctypes.c_double),
    ]


class MshaDstreamsJobsRouteStats(ctypes.Structure):
    _fields_ = [
        ("calls", ctypes.c_uint64),
        ("jobs", ctypes.c_uint64),
        ("launches_sort", ctypes.c_uint64),
        ("launches_rows", ctypes.c_uint64),
        ("launches_route", ctypes.c_uint64),
        ("launches_copy", ctypes.c_uint64),
        ("launches_chain", ctypes.c_uint64),
        ("launches_tail", ctypes.c_uint64),
        ("launches_write", ctypes.c_uint64),
        ("last_passes", ctypes.c_uint64),
        ("last_jobs", ctypes.c_uint64),
        ("last_routed", ctypes.c_uint64),
        ("last_routed_bytes", ctypes.c_uint64),
        ("last_kernel_ms", ctypes.c_double),
    ]


_setp = ctypes.c_void_p

# name -> (restype, argtypes)
SIGNATURES = {
    "msha_abi_version": (ctypes.c_uint32, []),
    "msha_build_id": (ctypes.c_char_p, []),
    "msha_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "msha_ctx_create": (ctypes.c_int, [ctypes.c_uint32, ctypes.POINTER(_ctxp)]),
    "msha_ctx_create_err": (ctypes.c_int, [ctypes.c_uint32, ctypes.POINTER(_ctxp), ctypes.c_char_p,
                                           ctypes.c_uint64]),
    "msha_ctx_destroy": (None, [_ctxp]),
    "msha_last_error": (ctypes.c_char_p, [_ctxp]),
    "msha_last_error_copy": (ctypes.c_uint64, [_ctxp, ctypes.c_char_p, ctypes.c_uint64]),
    "msha_get_stats": (ctypes.c_int, [_ctxp, ctypes.POINTER(MshaStats)]),
    "msha_shard_count": (ctypes.c_int, [_ctxp, ctypes.POINTER(ctypes.c_uint32)]),
    "msha_get_shard_stats": (ctypes.c_int, [_ctxp, ctypes.c_uint32, ctypes.POINTER(MshaShardStats)]),
    "msha_hash_actions": (ctypes.c_int, [_ctxp, _u8p, ctypes.c_uint64, _u64p, _u64p, ctypes.c_uint64,
                                         _u64p, ctypes.c_uint64, _u8p]),
    "msha_digest_batch": (ctypes.c_int, [_ctxp, _u8p, ctypes.c_uint64, _u64p, _u64p, ctypes.c_uint64,
                                         _u8p]),
    "msha_digest_of_digests": (ctypes.c_int, [_ctxp, _u8p, ctypes.c_uint64, _u32p, ctypes.c_uint64,
                                              _u64p, ctypes.c_uint64, _u8p]),
    "msha_digest_batch_device": (ctypes.c_int, [_ctxp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                ctypes.c_void_p]),
    "msha_digest_batch_device_planned": (ctypes.c_int, [_ctxp, ctypes.c_void_p, ctypes.c_void_p,
                                                        ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                                        ctypes.c_void_p, ctypes.c_void_p]),
    "msha_planned_read_plan": (ctypes.c_int, [_ctxp, ctypes.POINTER(MshaPlannedPlan), _u32p, ctypes.c_uint64, _u32p,
                                              ctypes.c_uint64]),
    "msha_digest_uniform_device": (ctypes.c_int, [_ctxp, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                                  ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]),
    "msha_digest_of_digests_device": (ctypes.c_int, [_ctxp, ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                     ctypes.c_void_p]),
    "msha_device_status": (ctypes.c_int, [_ctxp]),
    "msha_clock_probe": (ctypes.c_int, [_ctxp, ctypes.c_uint32, ctypes.POINTER(MshaClockInfo)]),
    "msha_set_kernel_policy": (ctypes.c_int, [_ctxp, ctypes.c_int]),
    "msha_pinned_alloc": (ctypes.c_int, [_ctxp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p)]),
    "msha_pinned_free": (ctypes.c_int, [_ctxp, ctypes.c_void_p]),
    "msha_blocks_for_len": (ctypes.c_uint64, [ctypes.c_uint64]),
    "msha_order_by_blocks": (ctypes.c_int, [_u64p, ctypes.c_uint64, _u32p]),
    "msha_partition_by_blocks": (ctypes.c_int, [_u64p, ctypes.c_uint64, ctypes.c_uint32, _u64p]),
    "msha_alias_first": (ctypes.c_int, [_u64p, _u64p, ctypes.c_uint64, _u64p]),
    "msha_streams_create": (ctypes.c_int, [_ctxp, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(_setp)]),
    "msha_streams_destroy": (None, [_setp]),
    "msha_streams_write": (ctypes.c_int, [_setp, _u8p, ctypes.c_uint64, _u64p, _u64p, _u64p, ctypes.c_uint64]),
    "msha_streams_sum": (ctypes.c_int, [_setp, _u64p, ctypes.c_uint64, _u8p]),
    "msha_streams_reset": (ctypes.c_int, [_setp, _u64p, ctypes.c_uint64]),
    "msha_streams_length": (ctypes.c_int, [_setp, _u64p, ctypes.c_uint64, _u64p]),
    "msha_streams_export": (ctypes.c_int, [_setp, _u64p, ctypes.c_uint64, _u8p]),
    "msha_streams_import": (ctypes.c_int, [_setp, _u64p, ctypes.c_uint64, _u8p]),
    "msha_streams_get_stats": (ctypes.c_int, [_setp, ctypes.POINTER(MshaStreamsStats)]),
    "msha_absorb_device": (ctypes.c_int, [_ctxp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "msha_absorb_chain_device": (ctypes.c_int, [_ctxp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "msha_finish_device": (ctypes.c_int, [_ctxp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                          ctypes.c_void_p]),
    "msha_hash_actions_device": (ctypes.c_int, [_ctxp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                ctypes.c_void_p, ctypes.c_void_p]),
    "msha_get_parts_stats": (ctypes.c_int, [_ctxp, ctypes.POINTER(MshaPartsStats)]),
    "msha_hash_actions_device_planned": (ctypes.c_int, [_ctxp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                        ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                        ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p,
                                                        ctypes.c_void_p]),
    "msha_get_parts_plan_stats": (ctypes.c_int, [_ctxp, ctypes.POINTER(MshaPartsPlanStats)]),
    "msha_parts_plan_read_order": (ctypes.c_int, [_ctxp, _u32p, ctypes.c_uint64, _u64p]),
    "msha_concat_lists_device": (ctypes.c_int, [_ctxp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "msha_get_concat_stats": (ctypes.c_int, [_ctxp, ctypes.POINTER(MshaConcatStats)]),
    "msha_verify_digests_device": (ctypes.c_int, [_ctxp, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                  ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                  ctypes.c_void_p]),
    "msha_get_verify_stats": (ctypes.c_int, [_ctxp, ctypes.POINTER(MshaVerifyStats)]),
    "msha_group_digests_device": (ctypes.c_int, [_ctxp, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                 ctypes.c_void_p, ctypes.c_void_p]),
    "msha_get_group_stats": (ctypes.c_int, [_ctxp, ctypes.POINTER(MshaGroupStats)]),
    "msha_dmap_create": (ctypes.c_int, [_ctxp, ctypes.c_uint64, ctypes.POINTER(_setp)]),
    "msha_dmap_destroy": (None, [_setp]),
    "msha_dmap_add_device": (ctypes.c_int, [_setp, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]),
    "msha_dmap_find_device": (ctypes.c_int, [_setp, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "msha_dmap_clear_device": (ctypes.c_int, [_setp, ctypes.c_void_p]),
    "msha_dmap_size": (ctypes.c_int, [_setp, _u64p]),
    "msha_dmap_read": (ctypes.c_int, [_setp, ctypes.c_uint64, ctypes.c_uint64, _u32p, _u8p, _u32p]),
    "msha_dmap_get_stats": (ctypes.c_int, [_setp, ctypes.POINTER(MshaDmapStats)]),
    "msha_dmap_create_voters": (ctypes.c_int, [_ctxp, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(_setp)]),
    "msha_dmap_vote_device": (ctypes.c_int, [_setp, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                             ctypes.c_void_p]),
    "msha_dmap_find_votes_device": (ctypes.c_int, [_setp, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.c_void_p]),
    "msha_dmap_read_voters": (ctypes.c_int, [_setp, ctypes.c_uint64, ctypes.c_uint64, _u32p]),
    "msha_dmap_get_vote_stats": (ctypes.c_int, [_setp, ctypes.POINTER(MshaDmapVoteStats)]),
    "msha_hash_actions_device_routed": (ctypes.c_int, [_ctxp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                       ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                       ctypes.c_uint64, ctypes.POINTER(MshaRouteOpts),
                                                       ctypes.c_void_p, ctypes.c_void_p]),
    "msha_get_parts_route_stats": (ctypes.c_int, [_ctxp, ctypes.POINTER(MshaPartsRouteStats)]),
    "msha_parts_route_read": (ctypes.c_int, [_ctxp, _u32p, ctypes.c_uint64, _u64p, _u64p]),
    "msha_parts_route_read_order": (ctypes.c_int, [_ctxp, _u32p, ctypes.c_uint64, _u64p]),
    "msha_dstreams_create": (ctypes.c_int, [_ctxp, ctypes.c_uint64, ctypes.POINTER(_setp)]),
    "msha_dstreams_destroy": (None, [_setp]),
    "msha_dstreams_write_device": (ctypes.c_int, [_setp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                  ctypes.c_void_p]),
    "msha_dstreams_sum_device": (ctypes.c_int, [_setp, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                ctypes.c_void_p]),
    "msha_dstreams_snap_device": (ctypes.c_int, [_setp, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                 ctypes.c_void_p]),
    "msha_dstreams_reset_device": (ctypes.c_int, [_setp, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "msha_dstreams_length": (ctypes.c_int, [_setp, _u64p, ctypes.c_uint64, _u64p]),
    "msha_dstreams_export": (ctypes.c_int, [_setp, _u64p, ctypes.c_uint64, _u8p]),
    "msha_dstreams_import": (ctypes.c_int, [_setp, _u64p, ctypes.c_uint64, _u8p]),
    "msha_dstreams_get_stats": (ctypes.c_int, [_setp, ctypes.POINTER(MshaDstreamsStats)]),
    "msha_dstreams_write_jobs_device": (ctypes.c_int, [_setp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                       ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
    "msha_dstreams_get_jobs_stats": (ctypes.c_int, [_setp, ctypes.POINTER(MshaDstreamsJobsStats)]),
    "msha_dstreams_jobs_read_order": (ctypes.c_int, [_setp, _u32p, ctypes.c_uint64, _u64p, _u64p]),
    "msha_dstreams_write_routed_device": (ctypes.c_int, [_setp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                         ctypes.POINTER(MshaRouteOpts), ctypes.c_void_p]),
    "msha_dstreams_get_route_stats": (ctypes.c_int, [_setp, ctypes.POINTER(MshaDstreamsRouteStats)]),
    "msha_dstreams_route_read": (ctypes.c_int, [_setp, _u32p, ctypes.c_uint64, _u64p, _u64p]),
    "msha_dstreams_write_jobs_routed_device": (ctypes.c_int, [_setp, ctypes.c_void_p, ctypes.c_void_p,
                                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                              ctypes.POINTER(MshaRouteOpts), ctypes.c_void_p]),
    "msha_dstreams_get_jobs_route_stats": (ctypes.c_int, [_setp, ctypes.POINTER(MshaDstreamsJobsRouteStats)]),
    "msha_dstreams_jobs_route_read": (ctypes.c_int, [_setp, _u32p, ctypes.c_uint64, _u64p, _u64p, _u32p,
                                                     ctypes.c_uint64, _u64p, _u64p]),
}

_lib = None


def header_symbols() -> list[str]:
    """Every function the public header declares."""
    with open(HEADER_PATH) as f:
        text = f.read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[\w\s\*]+?\b(msha_\w+)\s*\(", text, re.M)))


def lib() -> ctypes.CDLL:
    """Load libmirsha.so (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C mirbft_amd/csrc` (there is no CPU fallback)")
    # One HIP runtime per process: torch ships its own libamdhip64 (NEEDED as
    # "libamdhip64.so", SONAME libamdhip64.so.7). Loaded first, it satisfies our
    # NEEDED libamdhip64.so.7 by SONAME and both share it; loaded second, torch
    # would bring a second runtime and fail to initialise. So when torch is
    # installed it is imported before libmirsha.so is opened.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    if L.msha_abi_version() != ABI_VERSION:
        raise ImportError("libmirsha ABI version mismatch")
    _lib = L
    return L


# The files msha_build_id()'s src hash covers, in the Makefile's order (SRCS).
_SRC_FILES = ("sha256_device.hpp", "kernels.hpp", "kernels.hip", "plan.hip",
              os.path.join("..", "..", "include", "mirsha.h"),
              "msha_error.hpp", "host_plan.hpp", "ctx.hpp", "ctx.cpp", "host_small.hpp", "host_small.cpp",
              "host_pipeline.hpp", "host_pipeline.cpp", "host_direct.hpp", "host_direct.cpp",
              "host_entries.cpp", "device_batch.cpp",
              "stream_kernels.hip", "stream_pack.hpp", "ctx_access.hpp", "host_call.hpp", "workspace_rule.hpp",
              "call_workspace.hpp", "stream_state.hpp", "streams.cpp",
              "parts_gather.hpp", "parts_kernels.hip", "parts.cpp",
              "parts_digest.hpp", "parts_plan.hpp", "parts_plan.hip", "parts_plan.cpp",
              "parts_route.hpp", "parts_route.cpp",
              "stream_device.hpp", "stream_device.hip", "stream_device.cpp", "stream_jobs.hpp", "stream_jobs.hip",
              "stream_chain.hpp", "stream_chain.hip", "stream_write.hpp", "stream_jobs_route.hpp",
              "verify.hpp", "verify.hip", "verify.cpp",
              "group.hpp", "group.hip", "group.cpp",
              "dmap.hpp", "dmap.hip", "dmap.cpp", "dmap_vote.hpp", "dmap_vote.hip",
              "parts_concat.hpp", "parts_concat.hip", "parts_concat.cpp")


def source_id() -> str:
    """The src hash of the tree's sources, as the Makefile computes it for msha_build_id()."""
    import hashlib
    h = hashlib.sha256()
    for f in _SRC_FILES:
        with open(os.path.join(_HERE, "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def build_id() -> dict:
    """The loaded library's build: its src hash and flags, and whether it is the tree's own
    build (src equal to source_id() and no experiment's -D overrides in the flags)."""
    raw = lib().msha_build_id().decode()
    fields = dict(kv.split("=", 1) for kv in raw.split(";"))
    src, flags = fields.get("src", ""), fields.get("flags", "")
    tree = source_id()
    return {"id": raw, "src": src, "flags": flags, "tree_src": tree, "path": LIB_PATH,
            "matches_tree": (src == tree and not any(t.startswith("-D") for t in flags.split())
                             and os.path.realpath(LIB_PATH) == os.path.realpath(PRODUCT_LIB_PATH))}


def foreign_allowed() -> bool:
    """MSHA_ALLOW_FOREIGN_LIB=1: run on a library that is not the tree's build (A/B, diagnostics)."""
    return os.environ.get("MSHA_ALLOW_FOREIGN_LIB") == "1"


def require_tree_build(who: str) -> dict:
    """The loaded library's build_id(); raises unless it is the tree's own build or
    MSHA_ALLOW_FOREIGN_LIB=1 (results of an experiment's build must not be reported
    as the product's)."""
    b = build_id()
    if not b["matches_tree"] and not foreign_allowed():
        raise RuntimeError("%s: %s is not this tree's build (%s; tree src %s): rebuild it "
                           "(make -C mirbft_amd/csrc) or set MSHA_ALLOW_FOREIGN_LIB=1"
                           % (who, b["path"], b["id"], b["tree_src"]))
    return b
