"""Device digest maps: tallies that persist across calls in HBM (mirsha.h "Device digest
maps").

``DeviceDigestMap`` is the binding of ``msha_dmap_*``: the digest-keyed maps of the state
machine (a sequence's prepares and commits, a checkpoint's values, the request acks) kept
on the GPU from call to call. ``add_device`` counts the n digests of a call into the map:
each slot's key is (scope[i], 32 digest bytes), a key keeps the entry id it got when it
first occurred, its count runs on, and the call reports which keys crossed a threshold.
``find_device`` looks keys up without changing anything, ``clear_device`` empties the
map (one map a checkpoint window, cleared at garbage collection; there is no erase).
These three take torch tensors (``torch`` supplies device memory and streams only), only
enqueue, and capture into a HIP graph; ``size`` and ``read`` are synchronous and use numpy.

With ``max_voters`` > 0 the map is a VOTE MAP (mirsha.h "Device digest maps that count
voters"): a key's count is the number of distinct voters that voted for it, and the set of
voters lies in HBM beside the key. ``vote_device`` takes the place of ``add_device``
(which such a map refuses), ``find_votes_device`` also answers "has this voter voted for
this key", and ``read_voters`` returns the masks.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
from .engine import Engine, MshaError

NO_ID = 0xFFFFFFFF
RESULT_WORDS = 8
VOTE_RESULT_WORDS = 11
MAX_VOTERS = 1024
MAX_SLOTS = 1 << 30


class DeviceDigestMap:
    """A map of up to ``max_keys`` (scope, digest) keys on ``engine``'s first GPU."""

    def __init__(self, engine: Engine, max_keys: int, max_voters: int = 0):
        self._engine = engine
        self._lib = engine._lib
        self.max_keys = int(max_keys)
        self.max_voters = int(max_voters)
        if not 0 <= self.max_voters <= MAX_VOTERS:
            raise ValueError(f"max_voters must be 0 (a plain map) or 1 .. {MAX_VOTERS} (got {max_voters})")
        h = ctypes.c_void_p()
        if self.max_voters:
            engine._check(self._lib.msha_dmap_create_voters(engine._ctx, self.max_keys, self.max_voters,
                                                            ctypes.byref(h)))
        else:
            engine._check(self._lib.msha_dmap_create(engine._ctx, self.max_keys, ctypes.byref(h)))
        self._h = h
        if not hasattr(engine, "_sets"):
            engine._sets = []
        engine._sets.append(self)           # a map must go before its context, as a stream set must

    # -- lifecycle -------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.msha_dmap_destroy(self._h)
            self._h = None
            if self in getattr(self._engine, "_sets", []):
                self._engine._sets.remove(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> None:
        self._engine._check(rc)

    def _handle(self):
        if not getattr(self, "_h", None):
            raise MshaError(L.MSHA_ERR_INVALID_ARG, "device digest map is closed")
        return self._h

    # -- validation (before any C call: the ABI takes raw device pointers) -----
    def _device_index(self) -> int:
        dev = getattr(self._engine, "_dev_index", None)
        if dev is None:
            dev = self._engine._dev_index = self._engine._device_index()
        return dev

    def _check_tensors(self, **tensors) -> None:
        """Every tensor contiguous on the context's first GPU: bytes for digests, 4-byte
        integers for scope, voter, ids, counted, before, after, count, voted and crossed_slots,
        8-byte for result."""
        import torch
        dev = self._device_index()
        sizes = {"digests": 1, "scope": 4, "ids": 4, "before": 4, "after": 4, "count": 4, "crossed_slots": 4,
                 "result": 8, "voter": 4, "counted": 4, "voted": 4}
        for name, t in tensors.items():
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.device.index != dev:
                raise ValueError(f"{name} must be a torch tensor on cuda:{dev} (the context's first GPU)")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
            if t.element_size() != sizes[name] or t.is_floating_point():
                raise ValueError(f"{name} must hold {sizes[name]}-byte integers (got {t.dtype})")

    @staticmethod
    def _slots(digests, **per_slot) -> int:
        if digests.numel() % 32:
            raise ValueError(f"digests holds 32-byte rows (got {digests.numel()} bytes)")
        n = digests.numel() // 32
        if n > MAX_SLOTS:
            raise ValueError(f"digests holds {n} rows, at most 2^30 a call")
        for name, t in per_slot.items():
            if t is not None and t.numel() != n:
                raise ValueError(f"{name} has {t.numel()} entries, expected {n}")
        if digests.data_ptr() % L.MSHA_DEVICE_ALIGN:
            raise ValueError(f"digests must start on a {L.MSHA_DEVICE_ALIGN}-byte boundary")
        return n

    @staticmethod
    def _ptr(t):
        return None if t is None else t.data_ptr()

    def _voters(self) -> int:
        return getattr(self, "max_voters", 0)

    def _need_kind(self, votes: bool, what: str) -> None:
        """The C entries refuse the other kind of map; so does the wrapper, before C."""
        if votes and not self._voters():
            raise ValueError(f"{what}: this map keeps no voters: create it with max_voters > 0")
        if not votes and self._voters():
            raise ValueError(f"{what}: this is a vote map (max_voters={self._voters()}): use vote_device")

    # -- device calls ------------------------------------------------------
    def add_device(self, digests, ids, result, scope=None, threshold: int = 0, before=None, after=None,
                   crossed_slots=None, stream=None) -> None:
        """msha_dmap_add_device: slot i's key is (scope[i], or 0 with scope None, and the 32
        bytes digests[32 i ..]). ids[i] receives the key's entry id (kept if the map held
        the key, else numbered on in order of first occurrence), before[i] and after[i]
        (each may be None) its count before and after the call. crossed_slots (may be
        None) receives, in ascending order, the leader slot of each key whose count
        crossed threshold in this call, as far as it is long; result, eight 8-byte words:
        n, entries, added, full, crossed, listed, max_count, max_id. A call whose new keys
        do not all fit is refused whole: full is 1, every id 0xFFFFFFFF and the map as it
        was. Enqueue-only: nothing is read back here."""
        self._need_kind(False, "add_device")
        self._check_tensors(digests=digests, scope=scope, ids=ids, before=before, after=after,
                            crossed_slots=crossed_slots, result=result)
        n = self._slots(digests, scope=scope, ids=ids, before=before, after=after)
        if not 0 <= int(threshold) <= 0xFFFFFFFF:
            raise ValueError(f"threshold must fit 32 bits (got {threshold})")
        if result.numel() != RESULT_WORDS:
            raise ValueError(f"result must hold {RESULT_WORDS} words (got {result.numel()})")
        cap = 0 if crossed_slots is None else crossed_slots.numel()
        if n == 0:
            return
        h = self._handle()
        self._check(self._lib.msha_dmap_add_device(
            h, digests.data_ptr(), n, self._ptr(scope), int(threshold), ids.data_ptr(),
            self._ptr(before), self._ptr(after), crossed_slots.data_ptr() if cap else None, cap, result.data_ptr(),
            Engine._stream_ptr(stream)))

    def find_device(self, digests, ids, scope=None, count=None, stream=None) -> None:
        """msha_dmap_find_device: ids[i] and count[i] (count may be None) receive the entry
        id and the count of slot i's key, or 0xFFFFFFFF and 0 where the map does not hold
        it. One launch; the map is not changed."""
        self._check_tensors(digests=digests, scope=scope, ids=ids, count=count)
        n = self._slots(digests, scope=scope, ids=ids, count=count)
        if n == 0:
            return
        h = self._handle()
        self._check(self._lib.msha_dmap_find_device(
            h, digests.data_ptr(), n, self._ptr(scope), ids.data_ptr(), self._ptr(count),
            Engine._stream_ptr(stream)))

    def vote_device(self, digests, voter, ids, result, scope=None, threshold: int = 0, counted=None, before=None,
                    after=None, crossed_slots=None, stream=None) -> None:
        """msha_dmap_vote_device, on a vote map: slot i is voter[i]'s vote for the key
        (scope[i], digests[32 i ..]). counted[i] (may be None) is 1 iff voter[i] is below
        max_voters, no smaller slot of the call holds the same key and voter, and the
        voter had not voted for the key before the call. ids, before, after and
        crossed_slots as in add_device, the counts being distinct voters; result, eleven
        8-byte words: add_device's eight, then counted, repeats, bad_voters. Enqueue-only."""
        self._need_kind(True, "vote_device")
        self._check_tensors(digests=digests, scope=scope, voter=voter, ids=ids, counted=counted, before=before,
                            after=after, crossed_slots=crossed_slots, result=result)
        if voter is None:
            raise ValueError("voter must be a tensor of one 4-byte node id a slot")
        n = self._slots(digests, scope=scope, voter=voter, ids=ids, counted=counted, before=before, after=after)
        if not 0 <= int(threshold) <= 0xFFFFFFFF:
            raise ValueError(f"threshold must fit 32 bits (got {threshold})")
        if result.numel() != VOTE_RESULT_WORDS:
            raise ValueError(f"result must hold {VOTE_RESULT_WORDS} words (got {result.numel()})")
        cap = 0 if crossed_slots is None else crossed_slots.numel()
        if n == 0:
            return
        h = self._handle()
        self._check(self._lib.msha_dmap_vote_device(
            h, digests.data_ptr(), n, self._ptr(scope), voter.data_ptr(), int(threshold), ids.data_ptr(),
            self._ptr(counted), self._ptr(before), self._ptr(after), crossed_slots.data_ptr() if cap else None, cap,
            result.data_ptr(), Engine._stream_ptr(stream)))

    def find_votes_device(self, digests, voter, ids, voted, scope=None, count=None, stream=None) -> None:
        """msha_dmap_find_votes_device, on a vote map: find_device's answers, and voted[i] =
        1 iff the map holds slot i's key and voter[i] has voted for it (absent keys and
        voters at or past max_voters: 0). One launch; the map is not changed."""
        self._need_kind(True, "find_votes_device")
        self._check_tensors(digests=digests, scope=scope, voter=voter, ids=ids, count=count, voted=voted)
        if voter is None or voted is None:
            raise ValueError("voter and voted must be tensors of one 4-byte entry a slot")
        n = self._slots(digests, scope=scope, voter=voter, ids=ids, count=count, voted=voted)
        if n == 0:
            return
        h = self._handle()
        self._check(self._lib.msha_dmap_find_votes_device(
            h, digests.data_ptr(), n, self._ptr(scope), voter.data_ptr(), ids.data_ptr(), self._ptr(count),
            voted.data_ptr(), Engine._stream_ptr(stream)))

    def clear_device(self, stream=None) -> None:
        """msha_dmap_clear_device: the map empty again, ids start at 0. One launch."""
        h = self._handle()
        self._check(self._lib.msha_dmap_clear_device(h, Engine._stream_ptr(stream)))

    # -- synchronous, host memory ---------------------------------------------
    def size(self) -> int:
        """The number of keys in the map, once the device has finished."""
        e = ctypes.c_uint64(0)
        self._check(self._lib.msha_dmap_size(self._handle(), ctypes.byref(e)))
        return int(e.value)

    def read(self, first_id: int = 0, k: int | None = None):
        """(scope uint32 [k], digests uint8 [k, 32], count uint32 [k]) of the entries
        first_id .. first_id + k (k None: up to the last), once the device has finished."""
        if k is None:
            k = max(self.size() - int(first_id), 0)
        k = int(k)
        scope = np.zeros(k, dtype=np.uint32)
        digests = np.zeros((k, 32), dtype=np.uint8)
        count = np.zeros(k, dtype=np.uint32)
        u32p, u8p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)
        self._check(self._lib.msha_dmap_read(self._handle(), int(first_id), k, scope.ctypes.data_as(u32p),
                                             digests.ctypes.data_as(u8p), count.ctypes.data_as(u32p)))
        return scope, digests, count

    def read_voters(self, first_id: int = 0, k: int | None = None):
        """uint32 [k, words], words = ceil(max_voters / 32): the voter masks of the entries
        first_id .. first_id + k (k None: up to the last) of a vote map; bit v % 32 of word
        v / 32 is voter v. Once the device has finished."""
        self._need_kind(True, "read_voters")
        if k is None:
            k = max(self.size() - int(first_id), 0)
        k = int(k)
        words = (self._voters() + 31) // 32
        masks = np.zeros((k, words), dtype=np.uint32)
        self._check(self._lib.msha_dmap_read_voters(self._handle(), int(first_id), k,
                                                    masks.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        return masks

    def vote_stats(self) -> dict:
        """msha_dmap_get_vote_stats: votes, find_votes, the slots they took, launches (ten a
        vote, one a find_votes), max_voters, the mask's words and, under MSHA_PARTS_TIMING=1,
        the last vote call's kernel time."""
        s = L.MshaDmapVoteStats()
        self._check(self._lib.msha_dmap_get_vote_stats(self._handle(), ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in L.MshaDmapVoteStats._fields_}

    def stats(self) -> dict:
        """msha_dmap_get_stats: adds, finds, clears, the slots they took, launches (seven
        an add, one a find, one a clear), the table's positions and, under
        MSHA_PARTS_TIMING=1, the last call's kernel time."""
        s = L.MshaDmapStats()
        self._check(self._lib.msha_dmap_get_stats(self._handle(), ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in L.MshaDmapStats._fields_}
