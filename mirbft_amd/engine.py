"""Python handle on a libmirsha context (one or more GPUs).

``Engine`` is a thin, allocation-light wrapper over the C ABI
(include/mirsha.h). Host-memory calls take numpy arrays; device-resident calls
take torch tensors already on the GPU (``torch`` supplies device memory and
streams only -- all hashing happens in the HIP kernels of libmirsha.so).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from . import _lib as L


class MshaError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libmirsha error {code}: {msg}")
        self.code = code


def _p(a: np.ndarray, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def blocks_for_len(length: int) -> int:
    """FIPS 180-4 padded block count of an L-byte message (host-only helper)."""
    return int(L.lib().msha_blocks_for_len(int(length)))


def partition_by_blocks(lengths: np.ndarray, n_shards: int) -> np.ndarray:
    """Contiguous shard bounds with near-equal cumulative block counts."""
    lengths = np.ascontiguousarray(lengths, dtype=np.uint64)
    bounds = np.zeros(n_shards + 1, dtype=np.uint64)
    arg = lengths if lengths.size else np.zeros(1, dtype=np.uint64)
    rc = L.lib().msha_partition_by_blocks(_p(arg, ctypes.c_uint64), lengths.size, n_shards,
                                          _p(bounds, ctypes.c_uint64))
    if rc != L.MSHA_OK:
        raise MshaError(rc, "partition_by_blocks")
    return bounds


def order_by_blocks(lengths: np.ndarray) -> np.ndarray:
    """Permutation ordering messages by descending block count (for d_order)."""
    lengths = np.ascontiguousarray(lengths, dtype=np.uint64)
    order = np.zeros(max(lengths.size, 1), dtype=np.uint32)
    arg = lengths if lengths.size else np.zeros(1, dtype=np.uint64)
    rc = L.lib().msha_order_by_blocks(_p(arg, ctypes.c_uint64), lengths.size, _p(order, ctypes.c_uint32))
    if rc != L.MSHA_OK:
        raise MshaError(rc, "order_by_blocks")
    return order[: lengths.size]


def alias_first(off: np.ndarray, length: np.ndarray) -> np.ndarray:
    """first[i] = smallest j <= i with the same (off, len) (host-only helper)."""
    off = np.ascontiguousarray(off, dtype=np.uint64)
    length = np.ascontiguousarray(length, dtype=np.uint64)
    first = np.zeros(max(off.size, 1), dtype=np.uint64)
    a = off if off.size else np.zeros(1, dtype=np.uint64)
    b = length if length.size else np.zeros(1, dtype=np.uint64)
    rc = L.lib().msha_alias_first(_p(a, ctypes.c_uint64), _p(b, ctypes.c_uint64), off.size,
                                  _p(first, ctypes.c_uint64))
    if rc != L.MSHA_OK:
        raise MshaError(rc, "alias_first")
    return first[: off.size]


def device_count() -> int:
    n = ctypes.c_int(0)
    L.lib().msha_device_count(ctypes.byref(n))
    return n.value


class Engine:
    """A libmirsha context on the GPUs in ``device_mask`` (bit i = device i)."""

    def __init__(self, device_mask: int = 1):
        self._lib = L.lib()
        ctx = ctypes.c_void_p()
        err = ctypes.create_string_buffer(512)
        rc = self._lib.msha_ctx_create_err(device_mask, ctypes.byref(ctx), err, len(err))
        if rc != L.MSHA_OK:
            raise MshaError(rc, err.value.decode())
        self._ctx = ctx

    # -- lifecycle -------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_ctx", None):
            for st in list(getattr(self, "_sets", [])):   # a set must go before its context
                st.close()
            for p in getattr(self, "_pinned", []):
                self._lib.msha_pinned_free(self._ctx, p)
            self._pinned = []
            self._lib.msha_ctx_destroy(self._ctx)
            self._ctx = None

    def pinned_empty(self, nbytes: int) -> np.ndarray:
        """A uint8 numpy array in page-locked host memory (msha_pinned_alloc).
        Packing a batch into it (16-byte aligned message starts) lets
        digest_batch DMA it as is. Valid until close()."""
        p = ctypes.c_void_p()
        self._check(self._lib.msha_pinned_alloc(self._ctx, max(int(nbytes), 1), ctypes.byref(p)))
        if not hasattr(self, "_pinned"):
            self._pinned = []
        self._pinned.append(p.value)
        buf = (ctypes.c_uint8 * max(int(nbytes), 1)).from_address(p.value)
        return np.frombuffer(buf, dtype=np.uint8, count=int(nbytes))

    def pinned_free(self, a: np.ndarray) -> None:
        """Release a buffer from pinned_empty (by its base address)."""
        addr = a.__array_interface__["data"][0]
        if addr in getattr(self, "_pinned", []):
            self._pinned.remove(addr)
            self._check(self._lib.msha_pinned_free(self._ctx, addr))

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
        if rc != L.MSHA_OK:
            buf = ctypes.create_string_buffer(512)
            self._lib.msha_last_error_copy(self._ctx, buf, len(buf))   # under the context's lock
            raise MshaError(rc, buf.value.decode())

    def set_kernel_policy(self, policy: str) -> None:
        """"auto" (default), "lane" (one lane per message) or "coop" (cooperative chaining)."""
        code = {"auto": L.MSHA_KERNEL_AUTO, "lane": L.MSHA_KERNEL_LANE, "coop": L.MSHA_KERNEL_COOP}[policy]
        self._check(self._lib.msha_set_kernel_policy(self._ctx, code))

    def stats(self) -> dict:
        s = L.MshaStats()
        self._check(self._lib.msha_get_stats(self._ctx, ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in L.MshaStats._fields_}

    def shard_stats(self) -> list[dict]:
        """Per-GPU (per-shard) figures of the last host-memory call."""
        n = ctypes.c_uint32(0)
        self._check(self._lib.msha_shard_count(self._ctx, ctypes.byref(n)))
        out = []
        for i in range(n.value):
            s = L.MshaShardStats()
            self._check(self._lib.msha_get_shard_stats(self._ctx, i, ctypes.byref(s)))
            out.append({name: getattr(s, name) for name, _ in L.MshaShardStats._fields_})
        return out

    # -- host-memory entry points -----------------------------------------
    def digest_batch(self, arena: np.ndarray, off: np.ndarray, length: np.ndarray,
                     out: Optional[np.ndarray] = None) -> np.ndarray:
        """out[i] = SHA-256(arena[off[i] : off[i]+len[i]]) -> uint8 [n, 32]
        (``out``: an optional caller-owned C-contiguous uint8 [n, 32] result buffer)."""
        arena = np.ascontiguousarray(arena, dtype=np.uint8).reshape(-1)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        length = np.ascontiguousarray(length, dtype=np.uint64)
        n = off.size
        if out is None:
            out = np.empty((n, 32), dtype=np.uint8)
        elif out.shape != (n, 32) or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous uint8 array of shape (n, 32)")
        if n == 0:
            return out
        ap = arena if arena.size else np.zeros(1, dtype=np.uint8)
        self._check(self._lib.msha_digest_batch(self._ctx, _p(ap, ctypes.c_uint8), arena.size,
                                                _p(off, ctypes.c_uint64), _p(length, ctypes.c_uint64),
                                                n, _p(out, ctypes.c_uint8)))
        return out

    def hash_actions_packed(self, arena: np.ndarray, part_off: np.ndarray, part_len: np.ndarray,
                            action_part_begin: np.ndarray) -> np.ndarray:
        """msha_hash_actions over a packed arena -> uint8 [n_actions, 32]."""
        arena = np.ascontiguousarray(arena, dtype=np.uint8).reshape(-1)
        part_off = np.ascontiguousarray(part_off, dtype=np.uint64)
        part_len = np.ascontiguousarray(part_len, dtype=np.uint64)
        begin = np.ascontiguousarray(action_part_begin, dtype=np.uint64)
        n_actions = begin.size - 1
        out = np.empty((max(n_actions, 0), 32), dtype=np.uint8)
        if n_actions <= 0:
            return out
        ap = arena if arena.size else np.zeros(1, dtype=np.uint8)
        po = part_off if part_off.size else np.zeros(1, dtype=np.uint64)
        pl = part_len if part_len.size else np.zeros(1, dtype=np.uint64)
        self._check(self._lib.msha_hash_actions(self._ctx, _p(ap, ctypes.c_uint8), arena.size,
                                                _p(po, ctypes.c_uint64), _p(pl, ctypes.c_uint64),
                                                part_off.size, _p(begin, ctypes.c_uint64), n_actions,
                                                _p(out, ctypes.c_uint8)))
        return out

    def hash_actions(self, actions: Sequence[Sequence[bytes]]) -> list[bytes]:
        """One digest per action = SHA-256(concat(parts)), in input order."""
        arena, part_off, part_len, begin = pack_parts(actions)
        out = self.hash_actions_packed(arena, part_off, part_len, begin)
        return [bytes(r) for r in out]

    def digest_of_digests(self, table: np.ndarray, idx: np.ndarray, begin: np.ndarray) -> np.ndarray:
        table = np.ascontiguousarray(table, dtype=np.uint8).reshape(-1, 32)
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        begin = np.ascontiguousarray(begin, dtype=np.uint64)
        n = begin.size - 1
        out = np.empty((n, 32), dtype=np.uint8)
        if n <= 0:
            return out
        tp = table if table.size else np.zeros((1, 32), dtype=np.uint8)
        ip = idx if idx.size else np.zeros(1, dtype=np.uint32)
        self._check(self._lib.msha_digest_of_digests(self._ctx, _p(tp, ctypes.c_uint8), table.shape[0],
                                                     _p(ip, ctypes.c_uint32), idx.size,
                                                     _p(begin, ctypes.c_uint64), n,
                                                     _p(out, ctypes.c_uint8)))
        return out

    # -- device-resident entry points (torch tensors on the GPU) ----------
    @staticmethod
    def _stream_ptr(stream) -> Optional[int]:
        if stream is None:
            return None
        return int(getattr(stream, "cuda_stream", stream))

    def _device_index(self) -> int:
        n = ctypes.c_uint32(0)
        self._check(self._lib.msha_shard_count(self._ctx, ctypes.byref(n)))
        s = L.MshaShardStats()
        self._check(self._lib.msha_get_shard_stats(self._ctx, 0, ctypes.byref(s)))
        return int(s.device)

    def _check_device_args(self, n: int, out, **tensors) -> None:
        """The *_device entry points take raw device pointers: check here what
        the C ABI cannot -- every tensor contiguous on the context's first GPU,
        8-byte integers for off/len/begin, 4-byte for order/idx, out a uint8
        buffer of at least 32 n bytes -- so a mismatch raises instead of
        reading or writing out of bounds on the GPU."""
        import torch
        dev = getattr(self, "_dev_index", None)
        if dev is None:
            dev = self._dev_index = self._device_index()
        sizes = {"off": 8, "length": 8, "begin": 8, "order": 4, "idx": 4, "arena": 1, "table": 1,
                 "nblocks": 8, "prefix": 8, "state": 4, "part_off": 8, "part_len": 8, "list_begin": 8,
                 "action_list": 4, "dst": 1, "msg_off": 8, "msg_len": 8, "select": 4,
                 "got": 1, "expected": 1, "expected_idx": 4, "mask": 8, "bad_list": 4, "result": 8,
                 "digests": 1, "scope": 4, "first": 4, "group": 4, "members": 4, "group_first": 4,
                 "group_count": 4}
        for name, t in list(tensors.items()) + [("out", out)]:
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.device.index != dev:
                raise ValueError(f"{name} must be a torch tensor on cuda:{dev} (the context's first GPU)")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
            want = 1 if name == "out" else sizes[name]
            if t.element_size() != want or t.is_floating_point():
                raise ValueError(f"{name} must hold {want}-byte integers (got {t.dtype})")
        for name in ("off", "length", "order", "nblocks", "prefix", "action_list"):
            t = tensors.get(name)
            if t is not None and t.numel() != n:
                raise ValueError(f"{name} has {t.numel()} entries, expected {n}")
        t = tensors.get("state")
        if t is not None and t.numel() != 8 * n:
            raise ValueError(f"state has {t.numel()} words, expected {8 * n}")
        if out is not None and out.numel() < 32 * n:
            raise ValueError(f"out holds {out.numel()} bytes, needs {32 * n}")

    def digest_batch_device(self, arena, off, length, out, stream=None, order=None) -> None:
        self._check_device_args(off.numel(), out, arena=arena, off=off, length=length, order=order)
        self._check(self._lib.msha_digest_batch_device(self._ctx, arena.data_ptr(), off.data_ptr(),
                                                       length.data_ptr(),
                                                       None if order is None else order.data_ptr(),
                                                       off.numel(), out.data_ptr(), self._stream_ptr(stream)))

    def digest_batch_device_planned(self, arena, off, length, out, stream=None, fold: bool = False) -> None:
        """msha_digest_batch_device_planned: lane order (and, with fold, alias
        folding) planned on the GPU inside the call's launches."""
        self._check_device_args(off.numel(), out, arena=arena, off=off, length=length)
        self._check(self._lib.msha_digest_batch_device_planned(self._ctx, arena.data_ptr(), off.data_ptr(),
                                                               length.data_ptr(), off.numel(),
                                                               1 if fold else 0, out.data_ptr(),
                                                               self._stream_ptr(stream)))

    def planned_read_plan(self):
        """msha_planned_read_plan: the last digest_batch_device_planned call's plan ->
        (the counters as a dict, the lane order over all n positions, the early head's
        list). Waits for the device; a diagnostic. Before any planned call n is 0 and
        both arrays are empty."""
        p = L.MshaPlannedPlan()
        self._check(self._lib.msha_planned_read_plan(self._ctx, ctypes.byref(p), None, 0, None, 0))
        order = np.empty(p.n, dtype=np.uint32)
        longs = np.empty(min(p.long_listed, p.long_cap), dtype=np.uint32)
        if p.n:
            self._check(self._lib.msha_planned_read_plan(
                self._ctx, ctypes.byref(p), _p(order, ctypes.c_uint32) if order.size else None, order.size,
                _p(longs, ctypes.c_uint32) if longs.size else None, longs.size))
        return {name: getattr(p, name) for name, _ in L.MshaPlannedPlan._fields_}, order, longs

    def digest_uniform_device(self, arena, stride: int, msg_len: int, n: int, out, stream=None) -> None:
        self._check_device_args(n, out, arena=arena)
        self._check(self._lib.msha_digest_uniform_device(self._ctx, arena.data_ptr(), stride, msg_len, n,
                                                         out.data_ptr(), self._stream_ptr(stream)))

    def digest_of_digests_device(self, table, idx, begin, out, stream=None) -> None:
        self._check_device_args(begin.numel() - 1, out, table=table, idx=idx, begin=begin)
        self._check(self._lib.msha_digest_of_digests_device(self._ctx, table.data_ptr(), idx.data_ptr(),
                                                            begin.data_ptr(), begin.numel() - 1,
                                                            out.data_ptr(), self._stream_ptr(stream)))

    def absorb_device(self, state, arena, off, nblocks, stream=None) -> None:
        """msha_absorb_device: lane i compresses nblocks[i] whole 64-byte blocks at
        arena + off[i] into state[i] (n x 8 4-byte words, host order, in/out)."""
        self._check_device_args(off.numel(), None, state=state, arena=arena, off=off, nblocks=nblocks)
        self._check(self._lib.msha_absorb_device(self._ctx, state.data_ptr(), arena.data_ptr(), off.data_ptr(),
                                                 nblocks.data_ptr(), off.numel(), self._stream_ptr(stream)))

    def absorb_chain_device(self, state, arena, off, nblocks, stream=None) -> None:
        """msha_absorb_chain_device: absorb_device's arguments, rules and result on the
        eight-lane chain kernel -- eight GPU lanes a lane, for few, long lanes."""
        self._check_device_args(off.numel(), None, state=state, arena=arena, off=off, nblocks=nblocks)
        self._check(self._lib.msha_absorb_chain_device(self._ctx, state.data_ptr(), arena.data_ptr(),
                                                       off.data_ptr(), nblocks.data_ptr(), off.numel(),
                                                       self._stream_ptr(stream)))

    def finish_device(self, state, prefix, arena, off, length, out, stream=None) -> None:
        """msha_finish_device: out[i] = the digest of the message whose first prefix[i]
        bytes are in state[i] (None: the initial value, prefix None: 0) and whose last
        length[i] bytes are at arena + off[i]."""
        self._check_device_args(off.numel(), out, state=state, prefix=prefix, arena=arena, off=off, length=length)
        self._check(self._lib.msha_finish_device(self._ctx, None if state is None else state.data_ptr(),
                                                 None if prefix is None else prefix.data_ptr(),
                                                 arena.data_ptr(), off.data_ptr(), length.data_ptr(),
                                                 off.numel(), out.data_ptr(), self._stream_ptr(stream)))

    def hash_actions_device(self, arena, part_off, part_len, begin, out, stream=None, order=None) -> None:
        """msha_hash_actions_device: out[i] = SHA-256 of action i's parts
        [begin[i], begin[i+1]) back to back, part j = arena[part_off[j] : part_off[j] +
        part_len[j]] at any byte offset (pack_parts() output, uploaded as is, will do).
        The arena's base must be 16-byte aligned and MSHA_DEVICE_ARENA_SLACK readable
        bytes must follow the last part."""
        n = out.numel() // 32 if hasattr(out, "numel") else 0      # out is n x 32 bytes
        self._check_device_args(n, out, arena=arena, part_off=part_off, part_len=part_len, begin=begin,
                                order=order)
        if out.numel() != 32 * n:
            raise ValueError(f"out holds {out.numel()} bytes, not a multiple of 32")
        if begin.numel() != n + 1:
            raise ValueError(f"begin has {begin.numel()} entries, expected {n + 1} (out holds {n} digests)")
        if part_len.numel() != part_off.numel():
            raise ValueError(f"part_len has {part_len.numel()} entries, part_off {part_off.numel()}")
        if arena.data_ptr() % L.MSHA_DEVICE_ALIGN:
            raise ValueError(f"arena must start on a {L.MSHA_DEVICE_ALIGN}-byte boundary")
        if n == 0:
            return
        if arena.numel() == 0:          # nothing to read: an empty tensor has no address to pass
            arena = begin.new_zeros(2)
        if part_off.numel() == 0:       # every action has zero parts
            part_off = part_len = begin.new_zeros(2)
        self._check(self._lib.msha_hash_actions_device(self._ctx, arena.data_ptr(), part_off.data_ptr(),
                                                       part_len.data_ptr(), begin.data_ptr(),
                                                       None if order is None else order.data_ptr(), n,
                                                       out.data_ptr(), self._stream_ptr(stream)))

    def parts_stats(self) -> dict:
        """msha_get_parts_stats: calls, actions and launches of hash_actions_device, the
        last launch's lanes and (under MSHA_PARTS_TIMING=1) its kernel time."""
        s = L.MshaPartsStats()
        self._check(self._lib.msha_get_parts_stats(self._ctx, ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in L.MshaPartsStats._fields_}

    def hash_actions_device_planned(self, arena, part_off, part_len, list_begin, out, action_list=None,
                                    stream=None) -> None:
        """msha_hash_actions_device_planned: list l owns the parts [list_begin[l],
        list_begin[l+1]); out[i] = SHA-256 of the parts of list action_list[i] back to
        back (action_list None: of list i). Every list some action names is hashed
        once, the others not at all, and the lanes run in descending block-count
        class, planned on the GPU inside the call. Arena rules as hash_actions_device."""
        n = out.numel() // 32 if hasattr(out, "numel") else 0      # out is n x 32 bytes
        self._check_device_args(n, out, arena=arena, part_off=part_off, part_len=part_len,
                                list_begin=list_begin, action_list=action_list)
        if out.numel() != 32 * n:
            raise ValueError(f"out holds {out.numel()} bytes, not a multiple of 32")
        n_lists = list_begin.numel() - 1
        if n_lists < 0:
            raise ValueError("list_begin must have at least one entry")
        if action_list is None and n_lists != n:
            raise ValueError(f"list_begin has {list_begin.numel()} entries, expected {n + 1} (out holds {n} digests "
                             "and there is no action_list)")
        if part_len.numel() != part_off.numel():
            raise ValueError(f"part_len has {part_len.numel()} entries, part_off {part_off.numel()}")
        if arena.data_ptr() % L.MSHA_DEVICE_ALIGN:
            raise ValueError(f"arena must start on a {L.MSHA_DEVICE_ALIGN}-byte boundary")
        if n == 0:
            return
        if arena.numel() == 0:          # nothing to read: an empty tensor has no address to pass
            arena = list_begin.new_zeros(2)
        if part_off.numel() == 0:       # every list has zero parts
            part_off = part_len = list_begin.new_zeros(2)
        self._check(self._lib.msha_hash_actions_device_planned(
            self._ctx, arena.data_ptr(), part_off.data_ptr(), part_len.data_ptr(), list_begin.data_ptr(), n_lists,
            None if action_list is None else action_list.data_ptr(), n, 0, out.data_ptr(),
            self._stream_ptr(stream)))

    def parts_plan_stats(self) -> dict:
        """msha_get_parts_plan_stats: calls, actions, lists and launches of
        hash_actions_device_planned and, under MSHA_PARTS_TIMING=1, the last call's
        lanes (distinct lists hashed), blocks compressed and kernel time."""
        s = L.MshaPartsPlanStats()
        self._check(self._lib.msha_get_parts_plan_stats(self._ctx, ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in L.MshaPartsPlanStats._fields_}

    def parts_plan_order(self) -> np.ndarray:
        """msha_parts_plan_read_order: the last hash_actions_device_planned call's lane
        order (list indices, first lane first). Waits for the device; a diagnostic."""
        lanes = ctypes.c_uint64(0)
        self._check(self._lib.msha_parts_plan_read_order(self._ctx, None, 0, ctypes.byref(lanes)))
        order = np.empty(lanes.value, dtype=np.uint32)
        if lanes.value:
            self._check(self._lib.msha_parts_plan_read_order(self._ctx, _p(order, ctypes.c_uint32), order.size,
                                                             ctypes.byref(lanes)))
        return order[:lanes.value]

    def hash_actions_device_routed(self, arena, part_off, part_len, list_begin, out, action_list=None,
                                   stream=None, long_blocks: int = 0, max_long: int = 0,
                                   long_bytes: int = 0) -> None:
        """msha_hash_actions_device_routed: hash_actions_device_planned with the long
        lists found on the GPU inside the call, flattened into a buffer of the context's
        and hashed by the eight-lane chain kernel; the others run as lanes. A named list
        of long_blocks 64-byte blocks or more is long; at most max_long lists and
        long_bytes bytes are routed, and what finds no slot or no room stays a lane. 0
        takes a default (64 blocks, 16 x compute units, 32 MiB). Digests, errors and
        arena rules are hash_actions_device_planned's."""
        n = out.numel() // 32 if hasattr(out, "numel") else 0      # out is n x 32 bytes
        self._check_device_args(n, out, arena=arena, part_off=part_off, part_len=part_len,
                                list_begin=list_begin, action_list=action_list)
        if out.numel() != 32 * n:
            raise ValueError(f"out holds {out.numel()} bytes, not a multiple of 32")
        n_lists = list_begin.numel() - 1
        if n_lists < 0:
            raise ValueError("list_begin must have at least one entry")
        if action_list is None and n_lists != n:
            raise ValueError(f"list_begin has {list_begin.numel()} entries, expected {n + 1} (out holds {n} digests "
                             "and there is no action_list)")
        if part_len.numel() != part_off.numel():
            raise ValueError(f"part_len has {part_len.numel()} entries, part_off {part_off.numel()}")
        if arena.data_ptr() % L.MSHA_DEVICE_ALIGN:
            raise ValueError(f"arena must start on a {L.MSHA_DEVICE_ALIGN}-byte boundary")
        for name, v, top in (("long_blocks", long_blocks, 1 << 32), ("max_long", max_long, 1 << 32),
                             ("long_bytes", long_bytes, 1 << 64)):
            if not 0 <= int(v) < top:
                raise ValueError(f"{name} must be in [0, 2^{top.bit_length() - 1})")
        opts = L.MshaRouteOpts(int(long_blocks), int(max_long), int(long_bytes))
        if arena.numel() == 0 and n:    # nothing to read: an empty tensor has no address to pass
            arena = list_begin.new_zeros(2)
        if part_off.numel() == 0 and n:  # every list has zero parts
            part_off = part_len = list_begin.new_zeros(2)
        # (n == 0 goes to the library too, which launches nothing)
        self._check(self._lib.msha_hash_actions_device_routed(
            self._ctx, arena.data_ptr(), part_off.data_ptr(), part_len.data_ptr(), list_begin.data_ptr(), n_lists,
            None if action_list is None else action_list.data_ptr(), n, ctypes.byref(opts), out.data_ptr(),
            self._stream_ptr(stream)))

    def parts_route_stats(self) -> dict:
        """msha_get_parts_route_stats: calls, actions, lists and launches of
        hash_actions_device_routed and, under MSHA_PARTS_TIMING=1, the last call's lanes,
        their blocks, its routed lists, their bytes and the kernel time."""
        s = L.MshaPartsRouteStats()
        self._check(self._lib.msha_get_parts_route_stats(self._ctx, ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in L.MshaPartsRouteStats._fields_}

    def parts_route_lists(self):
        """msha_parts_route_read: (ids, bytes) of the last hash_actions_device_routed call
        -- the lists it routed, in no particular order, and the bytes of the flatten
        buffer they were given. Waits for the device; a diagnostic."""
        n, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self._lib.msha_parts_route_read(self._ctx, None, 0, ctypes.byref(n), ctypes.byref(b)))
        ids = np.empty(n.value, dtype=np.uint32)
        if n.value:
            self._check(self._lib.msha_parts_route_read(self._ctx, _p(ids, ctypes.c_uint32), ids.size,
                                                        ctypes.byref(n), ctypes.byref(b)))
        return ids[:n.value], int(b.value)

    def parts_route_order(self) -> np.ndarray:
        """msha_parts_route_read_order: the lane order of the last
        hash_actions_device_routed call (the lists that stayed lanes, first lane first).
        Waits for the device; a diagnostic."""
        lanes = ctypes.c_uint64(0)
        self._check(self._lib.msha_parts_route_read_order(self._ctx, None, 0, ctypes.byref(lanes)))
        order = np.empty(lanes.value, dtype=np.uint32)
        if lanes.value:
            self._check(self._lib.msha_parts_route_read_order(self._ctx, _p(order, ctypes.c_uint32), order.size,
                                                              ctypes.byref(lanes)))
        return order[:lanes.value]

    def concat_lists_device(self, arena, part_off, part_len, list_begin, dst, msg_off, msg_len, select=None,
                            stream=None) -> None:
        """msha_concat_lists_device: message k is list select[k] (select None: list k),
        its parts [list_begin[s], list_begin[s+1]) written back to back to dst at
        msg_off[k], msg_len[k] bytes, every start 16-byte aligned and the pad zeroed.
        (dst, msg_off, msg_len) then go to digest_batch_device as they are. A message
        that does not fit dst (with MSHA_DEVICE_ARENA_SLACK after it) or names an
        invalid list gets msg_off = msg_len = 0 and device_status() reports it. Arena
        rules as hash_actions_device; dst must start on a 16-byte boundary."""
        self._check_device_args(0, None, arena=arena, part_off=part_off, part_len=part_len,
                                list_begin=list_begin, dst=dst, msg_off=msg_off, msg_len=msg_len, select=select)
        n_lists = list_begin.numel() - 1
        if n_lists < 0:
            raise ValueError("list_begin must have at least one entry")
        n = n_lists if select is None else select.numel()
        if msg_off.numel() != n or msg_len.numel() != n:
            raise ValueError(f"msg_off and msg_len have {msg_off.numel()} and {msg_len.numel()} entries, "
                             f"expected {n}")
        if part_len.numel() != part_off.numel():
            raise ValueError(f"part_len has {part_len.numel()} entries, part_off {part_off.numel()}")
        if arena.data_ptr() % L.MSHA_DEVICE_ALIGN:
            raise ValueError(f"arena must start on a {L.MSHA_DEVICE_ALIGN}-byte boundary")
        if dst.data_ptr() % L.MSHA_DEVICE_ALIGN:
            raise ValueError(f"dst must start on a {L.MSHA_DEVICE_ALIGN}-byte boundary")
        if n == 0:
            return
        if arena.numel() == 0:          # nothing to read: an empty tensor has no address to pass
            arena = list_begin.new_zeros(2)
        if part_off.numel() == 0:       # every list has zero parts
            part_off = part_len = list_begin.new_zeros(2)
        dst_bytes = dst.numel()
        if dst_bytes == 0:              # everything is refused; still a valid address
            dst = list_begin.new_zeros(2)
        self._check(self._lib.msha_concat_lists_device(
            self._ctx, arena.data_ptr(), part_off.data_ptr(), part_len.data_ptr(), list_begin.data_ptr(), n_lists,
            None if select is None else select.data_ptr(), n, dst.data_ptr(), dst_bytes,
            msg_off.data_ptr(), msg_len.data_ptr(), self._stream_ptr(stream)))

    def concat_stats(self) -> dict:
        """msha_get_concat_stats: calls, lists and launches of concat_lists_device and,
        under MSHA_PARTS_TIMING=1, the last call's bytes laid out and kernel time."""
        s = L.MshaConcatStats()
        self._check(self._lib.msha_get_concat_stats(self._ctx, ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in L.MshaConcatStats._fields_}

    def verify_digests_device(self, got, expected, mask, result, expected_idx=None, bad_list=None,
                              stream=None) -> None:
        """msha_verify_digests_device: slot i of got (32 n bytes) is compared with row
        expected_idx[i] of expected (expected_idx None: row i, as many rows as slots). Bit
        i % 64 of mask[i // 64] is set where slot i differs, every one of the ceil(n / 64)
        words written; bad_list (may be None) receives the first min(bad, its length)
        differing slots in ascending order; result, five 8-byte words, receives n, bad,
        first_bad (n when none differs), listed and bad_index (slots whose index was out
        of range: they differ, and nothing of expected is read for them). Enqueue-only:
        nothing is read back here, and device_status() has nothing to report."""
        self._check_device_args(0, None, got=got, expected=expected, expected_idx=expected_idx, mask=mask,
                                bad_list=bad_list, result=result)
        if got.numel() % 32 or expected.numel() % 32:
            raise ValueError(f"got and expected hold 32-byte rows (got {got.numel()} and {expected.numel()} bytes)")
        n, n_expected = got.numel() // 32, expected.numel() // 32
        if expected_idx is None and n_expected != n:
            raise ValueError(f"without expected_idx expected must have as many rows as got ({n_expected} != {n})")
        if expected_idx is not None and expected_idx.numel() != n:
            raise ValueError(f"expected_idx has {expected_idx.numel()} entries, expected {n}")
        if mask.numel() < (n + 63) // 64:
            raise ValueError(f"mask holds {mask.numel()} words, needs {(n + 63) // 64}")
        if result.numel() != 5:
            raise ValueError(f"result must hold 5 words (got {result.numel()})")
        if got.data_ptr() % L.MSHA_DEVICE_ALIGN:
            raise ValueError(f"got must start on a {L.MSHA_DEVICE_ALIGN}-byte boundary")
        if expected.data_ptr() % L.MSHA_DEVICE_ALIGN:
            raise ValueError(f"expected must start on a {L.MSHA_DEVICE_ALIGN}-byte boundary")
        if n == 0:
            return
        if n_expected == 0:             # every index is out of range; still a valid address
            expected = got
        list_cap = 0 if bad_list is None else bad_list.numel()
        self._check(self._lib.msha_verify_digests_device(
            self._ctx, got.data_ptr(), n, expected.data_ptr(), n_expected,
            None if expected_idx is None else expected_idx.data_ptr(), mask.data_ptr(),
            bad_list.data_ptr() if list_cap else None, list_cap, result.data_ptr(), self._stream_ptr(stream)))

    def verify_stats(self) -> dict:
        """msha_get_verify_stats: calls, digests and launches of verify_digests_device,
        scan_words (mask words the scan takes a chunk: a constant) and, under
        MSHA_PARTS_TIMING=1, the last call's kernel time."""
        s = L.MshaVerifyStats()
        self._check(self._lib.msha_get_verify_stats(self._ctx, ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in L.MshaVerifyStats._fields_}

    def group_digests_device(self, digests, first, group, result, scope=None, members=None, group_first=None,
                             group_count=None, stream=None) -> None:
        """msha_group_digests_device: slot i's key is (scope[i], or 0 with scope None, and
        the 32 bytes digests[32 i ..]); slots with equal keys are one group. first[i]
        receives the smallest slot with slot i's key, group[i] the group's number (groups
        are numbered in order of first occurrence), members[i] (may be None) its size;
        group_first and group_count (both or neither; as long as each other) the leader
        and the size of the first min(groups, their length) groups; result, five 8-byte
        words, n, groups, listed, max_count and max_group (the smallest group id of that
        size). Enqueue-only: nothing is read back here, and device_status() has nothing
        to report."""
        self._check_device_args(0, None, digests=digests, scope=scope, first=first, group=group, members=members,
                                group_first=group_first, group_count=group_count, result=result)
        if digests.numel() % 32:
            raise ValueError(f"digests holds 32-byte rows (got {digests.numel()} bytes)")
        n = digests.numel() // 32
        for name, t in (("scope", scope), ("first", first), ("group", group), ("members", members)):
            if t is not None and t.numel() != n:
                raise ValueError(f"{name} has {t.numel()} entries, expected {n}")
        if (group_first is None) != (group_count is None):
            raise ValueError("group_first and group_count go together: both or neither")
        group_cap = 0 if group_first is None else group_first.numel()
        if group_cap and group_count.numel() != group_cap:
            raise ValueError(f"group_count has {group_count.numel()} entries, group_first {group_cap}")
        if result.numel() != 5:
            raise ValueError(f"result must hold 5 words (got {result.numel()})")
        if digests.data_ptr() % L.MSHA_DEVICE_ALIGN:
            raise ValueError(f"digests must start on a {L.MSHA_DEVICE_ALIGN}-byte boundary")
        if n == 0:
            return
        self._check(self._lib.msha_group_digests_device(
            self._ctx, digests.data_ptr(), n, None if scope is None else scope.data_ptr(), first.data_ptr(),
            group.data_ptr(), None if members is None else members.data_ptr(),
            group_first.data_ptr() if group_cap else None, group_count.data_ptr() if group_cap else None, group_cap,
            result.data_ptr(), self._stream_ptr(stream)))

    def group_stats(self) -> dict:
        """msha_get_group_stats: calls, digests and launches (six a call) of
        group_digests_device, the last call's table positions and, under
        MSHA_PARTS_TIMING=1, its kernel time."""
        s = L.MshaGroupStats()
        self._check(self._lib.msha_get_group_stats(self._ctx, ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in L.MshaGroupStats._fields_}

    def clock_probe(self, blocks_per_lane: int = 48) -> dict:
        """msha_clock_probe: the clock the first GPU holds under the hash
        kernels' instruction mix (in-kernel s_memtime / s_memrealtime)."""
        c = L.MshaClockInfo()
        self._check(self._lib.msha_clock_probe(self._ctx, int(blocks_per_lane), ctypes.byref(c)))
        return {name: getattr(c, name) for name, _ in L.MshaClockInfo._fields_}

    def device_status(self) -> None:
        self._check(self._lib.msha_device_status(self._ctx))


def pack_parts(actions: Sequence[Sequence[bytes]]):
    """Pack [][]byte parts into (arena, part_off, part_len, action_part_begin),
    the layout a cgo adapter hands to msha_hash_actions."""
    parts = [bytes(p) for a in actions for p in a]
    lens = np.fromiter((len(p) for p in parts), dtype=np.uint64, count=len(parts))
    offs = np.zeros(len(parts), dtype=np.uint64)
    if len(parts) > 1:
        offs[1:] = np.cumsum(lens)[:-1]
    arena = np.frombuffer(b"".join(parts), dtype=np.uint8)
    begin = np.zeros(len(actions) + 1, dtype=np.uint64)
    if actions:
        begin[1:] = np.cumsum([len(a) for a in actions])
    return arena, offs, lens, begin
