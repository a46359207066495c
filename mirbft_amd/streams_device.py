"""Device stream sets: resumable SHA-256 streams written and summed in HBM (mirsha.h
"Device stream sets").

``DeviceStreamSet`` is the binding of ``msha_dstreams_*``: ``n`` independent
``hash.Hash`` states whose chaining state, 64-byte buffer and length all live on the
GPU. ``write_device`` appends parts that already sit in device memory (at any byte
offset of an arena), ``sum_device`` / ``snap_device`` / ``reset_device`` are
NodeState's Sum(nil), Snap and a fresh hash (pkg/testengine/recorder.go:288-359); each
is one kernel launch on the caller's stream with no host wait, so a sequence of them
captures into a HIP graph. ``write_jobs_device`` is ``StreamSet.write``'s job list in
device memory -- jobs in call order, a stream named any number of times -- grouped by
stream on the GPU inside the call: several launches, still on the caller's stream and
capturable once its workspace exists. ``write_routed_device`` is ``write_device`` with the
rows that compress many blocks found on the GPU and run on the eight-lane chain, eight
lanes a stream instead of one; ``write_jobs_routed_device`` is the two in one call, jobs
in call order whose long streams take the chain. The device calls take torch tensors (``torch`` supplies
device memory and streams only); ``lengths``, ``export_state`` and ``import_state``
are synchronous and use numpy, in the layout ``StreamSet`` exports.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
from .engine import Engine, MshaError, _p

STATE_BYTES = L.MSHA_STREAM_STATE_BYTES


class DeviceStreamSet:
    """``n`` streams in New() state on ``engine``'s first GPU."""

    def __init__(self, engine: Engine, n: int):
        self._engine = engine
        self._lib = engine._lib
        self.n = int(n)
        h = ctypes.c_void_p()
        engine._check(self._lib.msha_dstreams_create(engine._ctx, self.n, ctypes.byref(h)))
        self._h = h
        if not hasattr(engine, "_sets"):
            engine._sets = []
        engine._sets.append(self)

    # -- lifecycle -------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.msha_dstreams_destroy(self._h)
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
            raise MshaError(L.MSHA_ERR_INVALID_ARG, "device stream set is closed")
        return self._h

    # -- validation (before any C call: the ABI takes raw device pointers) -----
    def _device_index(self) -> int:
        dev = getattr(self._engine, "_dev_index", None)
        if dev is None:
            dev = self._engine._dev_index = self._engine._device_index()
        return dev

    def _check_tensors(self, **tensors) -> None:
        """Every tensor contiguous on the context's first GPU, 8-byte integers for
        part_off / part_len / row_part_begin, 4-byte for rows, bytes for arena / out."""
        import torch
        dev = self._device_index()
        sizes = {"arena": 1, "out": 1, "part_off": 8, "part_len": 8, "row_part_begin": 8, "rows": 4,
                 "job_stream": 4, "job_off": 8, "job_len": 8}
        for name, t in tensors.items():
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.device.index != dev:
                raise ValueError(f"{name} must be a torch tensor on cuda:{dev} (the context's first GPU)")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
            if t.element_size() != sizes[name] or t.is_floating_point():
                raise ValueError(f"{name} must hold {sizes[name]}-byte integers (got {t.dtype})")

    def _n_rows(self, rows) -> int:
        return self.n if rows is None else rows.numel()

    @staticmethod
    def _ptr(t):
        return None if t is None else t.data_ptr()

    # -- device calls ------------------------------------------------------
    def write_device(self, arena, part_off, part_len, row_part_begin, rows=None, stream=None) -> None:
        """Row r -- stream rows[r], or stream r of all n when rows is None -- appends the
        parts [row_part_begin[r], row_part_begin[r+1]) back to back, part j =
        arena[part_off[j] : part_off[j] + part_len[j]] at any byte offset. A stream may
        be named at most once per call (not detected). The arena's base must be 16-byte
        aligned and MSHA_DEVICE_ARENA_SLACK readable bytes must follow the last part."""
        self._check_tensors(arena=arena, part_off=part_off, part_len=part_len, row_part_begin=row_part_begin,
                            rows=rows)
        n_rows = self._n_rows(rows)
        if row_part_begin.numel() != n_rows + 1:
            raise ValueError(f"row_part_begin has {row_part_begin.numel()} entries, expected {n_rows + 1}")
        if part_len.numel() != part_off.numel():
            raise ValueError(f"part_len has {part_len.numel()} entries, part_off {part_off.numel()}")
        if arena.data_ptr() % L.MSHA_DEVICE_ALIGN:
            raise ValueError(f"arena must start on a {L.MSHA_DEVICE_ALIGN}-byte boundary")
        if n_rows == 0:
            return
        if arena.numel() == 0:          # nothing to read: an empty tensor has no address to pass
            arena = row_part_begin.new_zeros(2)
        if part_off.numel() == 0:       # every row has zero parts
            part_off = part_len = row_part_begin.new_zeros(2)
        self._check(self._lib.msha_dstreams_write_device(
            self._handle(), arena.data_ptr(), part_off.data_ptr(), part_len.data_ptr(), row_part_begin.data_ptr(),
            self._ptr(rows), n_rows, Engine._stream_ptr(stream)))

    def write_routed_device(self, arena, part_off, part_len, row_part_begin, rows=None, stream=None,
                            long_blocks: int = 0, max_long: int = 0, long_bytes: int = 0) -> None:
        """write_device with its long rows found on the GPU inside the call and run on the
        eight-lane chain: a row whose write compresses long_blocks 64-byte blocks or more
        is flattened behind its stream's buffered bytes into a buffer of the set's and
        absorbed with eight lanes; the others are lanes as in write_device. At most
        max_long rows and long_bytes bytes are routed, and a row that finds no slot or no
        room stays a lane. 0 takes a default (64 blocks, 16 x compute units, 32 MiB).
        State, buffer, length, errors and arena rules are write_device's; six launches,
        all on ``stream``."""
        self._check_tensors(arena=arena, part_off=part_off, part_len=part_len, row_part_begin=row_part_begin,
                            rows=rows)
        n_rows = self._n_rows(rows)
        if row_part_begin.numel() != n_rows + 1:
            raise ValueError(f"row_part_begin has {row_part_begin.numel()} entries, expected {n_rows + 1}")
        if part_len.numel() != part_off.numel():
            raise ValueError(f"part_len has {part_len.numel()} entries, part_off {part_off.numel()}")
        if arena.data_ptr() % L.MSHA_DEVICE_ALIGN:
            raise ValueError(f"arena must start on a {L.MSHA_DEVICE_ALIGN}-byte boundary")
        for name, v, top in (("long_blocks", long_blocks, 1 << 32), ("max_long", max_long, 1 << 32),
                             ("long_bytes", long_bytes, 1 << 64)):
            if not 0 <= int(v) < top:
                raise ValueError(f"{name} must be in [0, 2^{top.bit_length() - 1})")
        if n_rows == 0:
            return
        opts = L.MshaRouteOpts(int(long_blocks), int(max_long), int(long_bytes))
        if arena.numel() == 0:          # nothing to read: an empty tensor has no address to pass
            arena = row_part_begin.new_zeros(2)
        if part_off.numel() == 0:       # every row has zero parts
            part_off = part_len = row_part_begin.new_zeros(2)
        self._check(self._lib.msha_dstreams_write_routed_device(
            self._handle(), arena.data_ptr(), part_off.data_ptr(), part_len.data_ptr(), row_part_begin.data_ptr(),
            self._ptr(rows), n_rows, ctypes.byref(opts), Engine._stream_ptr(stream)))

    def route_stats(self) -> dict:
        """The counters of write_routed_device (stats() and jobs_stats() count none of its
        calls); last_routed, last_routed_bytes and last_kernel_ms only under
        MSHA_PARTS_TIMING=1."""
        s = L.MshaDstreamsRouteStats()
        self._check(self._lib.msha_dstreams_get_route_stats(self._handle(), ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in L.MshaDstreamsRouteStats._fields_}

    def routed_rows(self):
        """(rows, bytes) of the last write_routed_device (waits for the device): the row
        indices it routed, in no particular order, and the bytes of the flatten buffer
        they were given. A diagnostic."""
        n, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self._lib.msha_dstreams_route_read(self._handle(), None, 0, ctypes.byref(n), ctypes.byref(b)))
        ids = np.empty(n.value, dtype=np.uint32)
        if n.value:
            self._check(self._lib.msha_dstreams_route_read(self._handle(), _p(ids, ctypes.c_uint32), ids.size,
                                                           ctypes.byref(n), ctypes.byref(b)))
        return ids[:n.value], b.value

    def write_jobs_device(self, arena, job_stream, job_off, job_len, stream=None) -> None:
        """StreamSet.write's job list in device memory: for j in call order, stream
        job_stream[j] appends arena[job_off[j] : job_off[j] + job_len[j]]. A stream may
        be named any number of times; its chunks append in job order. The jobs are
        grouped by stream on the GPU inside the call (several kernel launches, all on
        ``stream``). A job whose stream is >= n is dropped and reported by
        ``Engine.device_status()``. The arena rules are write_device's."""
        self._check_tensors(arena=arena, job_stream=job_stream, job_off=job_off, job_len=job_len)
        n_jobs = job_stream.numel()
        if job_off.numel() != n_jobs or job_len.numel() != n_jobs:
            raise ValueError(f"job_stream has {n_jobs} entries, job_off {job_off.numel()}, job_len {job_len.numel()}")
        if arena.data_ptr() % L.MSHA_DEVICE_ALIGN:
            raise ValueError(f"arena must start on a {L.MSHA_DEVICE_ALIGN}-byte boundary")
        if n_jobs == 0:
            return
        if arena.numel() == 0:          # nothing to read: an empty tensor has no address to pass
            arena = job_off.new_zeros(2)
        self._check(self._lib.msha_dstreams_write_jobs_device(
            self._handle(), arena.data_ptr(), job_stream.data_ptr(), job_off.data_ptr(), job_len.data_ptr(), n_jobs,
            Engine._stream_ptr(stream)))

    def jobs_stats(self) -> dict:
        """The counters of write_jobs_device (stats() counts none of its calls)."""
        s = L.MshaDstreamsJobsStats()
        self._check(self._lib.msha_dstreams_get_jobs_stats(self._handle(), ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in L.MshaDstreamsJobsStats._fields_}

    def jobs_order(self):
        """(order, n_valid) of the last write_jobs_device (waits for the device): order[p]
        is the job applied p-th -- argsort(min(job_stream, n), stable) -- and the first
        n_valid of them name a stream of the set."""
        k = self.jobs_stats()["last_jobs"]
        order = np.zeros(max(k, 1), dtype=np.uint32)
        n_jobs, n_valid = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.msha_dstreams_jobs_read_order(self._handle(), _p(order, ctypes.c_uint32), k,
                                                            ctypes.byref(n_jobs), ctypes.byref(n_valid)))
        return order[:n_jobs.value], n_valid.value

    def write_jobs_routed_device(self, arena, job_stream, job_off, job_len, stream=None,
                                 long_blocks: int = 0, max_long: int = 0, long_bytes: int = 0) -> None:
        """write_jobs_device with its long streams on the eight-lane chain: the jobs are
        grouped by stream on the GPU as there, then written as write_routed_device writes
        the grouped CSR -- a stream whose valid jobs make its write compress long_blocks
        64-byte blocks or more is flattened and absorbed with eight lanes, the others are
        lanes. At most max_long streams and long_bytes bytes are routed; 0 takes a
        default (64 blocks, 16 x compute units, 32 MiB). State, buffer, length, dropped
        jobs and arena rules are write_jobs_device's whatever the three hold; 3 x passes +
        8 launches, all on ``stream``."""
        self._check_tensors(arena=arena, job_stream=job_stream, job_off=job_off, job_len=job_len)
        n_jobs = job_stream.numel()
        if job_off.numel() != n_jobs or job_len.numel() != n_jobs:
            raise ValueError(f"job_stream has {n_jobs} entries, job_off {job_off.numel()}, job_len {job_len.numel()}")
        if arena.data_ptr() % L.MSHA_DEVICE_ALIGN:
            raise ValueError(f"arena must start on a {L.MSHA_DEVICE_ALIGN}-byte boundary")
        for name, v, top in (("long_blocks", long_blocks, 1 << 32), ("max_long", max_long, 1 << 32),
                             ("long_bytes", long_bytes, 1 << 64)):
            if not 0 <= int(v) < top:
                raise ValueError(f"{name} must be in [0, 2^{top.bit_length() - 1})")
        if n_jobs == 0:
            return
        opts = L.MshaRouteOpts(int(long_blocks), int(max_long), int(long_bytes))
        if arena.numel() == 0:          # nothing to read: an empty tensor has no address to pass
            arena = job_off.new_zeros(2)
        self._check(self._lib.msha_dstreams_write_jobs_routed_device(
            self._handle(), arena.data_ptr(), job_stream.data_ptr(), job_off.data_ptr(), job_len.data_ptr(), n_jobs,
            ctypes.byref(opts), Engine._stream_ptr(stream)))

    def jobs_route_stats(self) -> dict:
        """The counters of write_jobs_routed_device (stats(), jobs_stats() and route_stats()
        count none of its calls); last_routed, last_routed_bytes and last_kernel_ms only
        under MSHA_PARTS_TIMING=1."""
        s = L.MshaDstreamsJobsRouteStats()
        self._check(self._lib.msha_dstreams_get_jobs_route_stats(self._handle(), ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in L.MshaDstreamsJobsRouteStats._fields_}

    def jobs_route_read(self):
        """(order, n_valid, routed_streams, routed_bytes) of the last
        write_jobs_routed_device (waits for the device): the job order and its count of
        valid jobs as jobs_order() gives them, the streams it routed, in no particular
        order, and the bytes of the flatten buffer they were given. A diagnostic;
        jobs_order() and routed_rows() are not touched by that call."""
        n_jobs, n_valid, n_routed, nbytes = (ctypes.c_uint64(0) for _ in range(4))
        f = self._lib.msha_dstreams_jobs_route_read
        self._check(f(self._handle(), None, 0, ctypes.byref(n_jobs), ctypes.byref(n_valid), None, 0,
                      ctypes.byref(n_routed), ctypes.byref(nbytes)))
        order = np.zeros(max(n_jobs.value, 1), dtype=np.uint32)
        ids = np.zeros(max(n_routed.value, 1), dtype=np.uint32)
        k, m = n_jobs.value, n_routed.value
        if k or m:
            self._check(f(self._handle(), _p(order, ctypes.c_uint32), k, ctypes.byref(n_jobs), ctypes.byref(n_valid),
                          _p(ids, ctypes.c_uint32), m, ctypes.byref(n_routed), ctypes.byref(nbytes)))
        return order[:k], n_valid.value, ids[:m], nbytes.value

    def _finish(self, fn, out, rows, stream) -> None:
        self._check_tensors(out=out, rows=rows)
        n_rows = self._n_rows(rows)
        if out.numel() < 32 * n_rows:
            raise ValueError(f"out holds {out.numel()} bytes, needs {32 * n_rows}")
        if n_rows == 0:
            return
        self._check(getattr(self._lib, fn)(self._handle(), self._ptr(rows), n_rows, out.data_ptr(),
                                           Engine._stream_ptr(stream)))

    def sum_device(self, out, rows=None, stream=None) -> None:
        """out[32 r] = SHA-256 of everything written to row r's stream; no stream changes."""
        self._finish("msha_dstreams_sum_device", out, rows, stream)

    def snap_device(self, out, rows=None, stream=None) -> None:
        """NodeState.Snap: out[32 r] = Sum(nil); the stream then is New() followed by
        Write(that sum)."""
        self._finish("msha_dstreams_snap_device", out, rows, stream)

    def reset_device(self, rows=None, stream=None) -> None:
        """The rows' streams return to New()."""
        self._check_tensors(rows=rows)
        n_rows = self._n_rows(rows)
        if n_rows == 0:
            return
        self._check(self._lib.msha_dstreams_reset_device(self._handle(), self._ptr(rows), n_rows,
                                                         Engine._stream_ptr(stream)))

    # -- synchronous, host memory ------------------------------------------
    def _ids(self, ids):
        if ids is None:
            return None, self.n, None
        a = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        keep = a if a.size else np.zeros(1, dtype=np.uint64)
        return _p(keep, ctypes.c_uint64), a.size, keep

    def lengths(self, ids=None) -> np.ndarray:
        """Bytes written to each stream so far (waits for the device)."""
        ptr, k, keep = self._ids(ids)
        out = np.zeros(max(k, 1), dtype=np.uint64)
        self._check(self._lib.msha_dstreams_length(self._handle(), ptr, k, _p(out, ctypes.c_uint64)))
        return out[:k]

    def export_state(self, ids=None) -> np.ndarray:
        """uint8 [k, 108]: each stream's state in StreamSet.export_state's layout (waits
        for the device)."""
        ptr, k, keep = self._ids(ids)
        out = np.zeros((max(k, 1), STATE_BYTES), dtype=np.uint8)
        self._check(self._lib.msha_dstreams_export(self._handle(), ptr, k, _p(out, ctypes.c_uint8)))
        return out[:k]

    def import_state(self, ids, states) -> None:
        """Streams ids[j] take the exported state states[j] (uint8 [k, 108] or bytes),
        from this kind of set or from a StreamSet."""
        if isinstance(states, (bytes, bytearray)):
            states = np.frombuffer(bytes(states), dtype=np.uint8)
        states = np.ascontiguousarray(states, dtype=np.uint8).reshape(-1, STATE_BYTES)
        ptr, k, keep = self._ids(ids)
        if states.shape[0] != k:
            raise ValueError("one %d-byte state per id" % STATE_BYTES)
        sp = states if states.size else np.zeros((1, STATE_BYTES), dtype=np.uint8)
        self._check(self._lib.msha_dstreams_import(self._handle(), ptr, k, _p(sp, ctypes.c_uint8)))

    def stats(self) -> dict:
        s = L.MshaDstreamsStats()
        self._check(self._lib.msha_dstreams_get_stats(self._handle(), ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in L.MshaDstreamsStats._fields_}


__all__ = ["DeviceStreamSet", "STATE_BYTES"]
