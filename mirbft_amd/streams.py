"""Stream sets: many resumable SHA-256 streams on one GPU (mirsha.h "Stream sets").

``StreamSet`` is the binding of ``msha_streams_*``: ``n`` independent
``hash.Hash`` states -- the streaming half of the reference's ``processor.Hasher``
(``New() hash.Hash``, pkg/processor/serial.go:21-23) as NodeState.Apply / Snap use
it (pkg/testengine/recorder.go:288-359). Writes to many streams go to the GPU in
one call; each stream keeps its chaining state there and its partial block on the
host. One stream is one GPU lane, so the gain is across streams: a lone stream
runs at one lane's rate.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from . import _lib as L
from .engine import Engine, MshaError, _p

STATE_BYTES = L.MSHA_STREAM_STATE_BYTES


class StreamSet:
    """``n`` streams in New() state on ``engine``'s first GPU. ``staging_bytes``
    bounds the pinned and device staging one piece of a write uses (0: 64 MiB)."""

    def __init__(self, engine: Engine, n: int, staging_bytes: int = 0):
        self._engine = engine
        self._lib = engine._lib
        self.n = int(n)
        h = ctypes.c_void_p()
        engine._check(self._lib.msha_streams_create(engine._ctx, self.n, int(staging_bytes), ctypes.byref(h)))
        self._h = h
        if not hasattr(engine, "_sets"):
            engine._sets = []
        engine._sets.append(self)

    # -- lifecycle -------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.msha_streams_destroy(self._h)
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
            raise MshaError(L.MSHA_ERR_INVALID_ARG, "stream set is closed")
        return self._h

    def _ids(self, ids):
        """(pointer or None, k) for an id list; None means every stream."""
        if ids is None:
            return None, self.n, None
        a = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        keep = a if a.size else np.zeros(1, dtype=np.uint64)
        return _p(keep, ctypes.c_uint64), a.size, keep

    # -- Write -----------------------------------------------------------
    def write_packed(self, arena: np.ndarray, ids: np.ndarray, off: np.ndarray, length: np.ndarray) -> None:
        """For j in order, stream ids[j] appends arena[off[j] : off[j]+length[j]]
        (msha_streams_write; no per-item Python work)."""
        arena = np.ascontiguousarray(arena, dtype=np.uint8).reshape(-1)
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        off = np.ascontiguousarray(off, dtype=np.uint64).reshape(-1)
        length = np.ascontiguousarray(length, dtype=np.uint64).reshape(-1)
        if not (ids.size == off.size == length.size):
            raise ValueError("ids, off and length must have one entry per chunk")
        k = ids.size
        ap = arena if arena.size else np.zeros(1, dtype=np.uint8)
        z = np.zeros(1, dtype=np.uint64)
        self._check(self._lib.msha_streams_write(self._handle(), _p(ap, ctypes.c_uint8), arena.size,
                                                 _p(ids if k else z, ctypes.c_uint64),
                                                 _p(off if k else z, ctypes.c_uint64),
                                                 _p(length if k else z, ctypes.c_uint64), k))

    def write(self, ids: Sequence[int], chunks: Sequence[bytes]) -> None:
        """Stream ids[j] appends chunks[j], in order (an id may repeat)."""
        if len(ids) != len(chunks):
            raise ValueError("one chunk per id")
        lens = np.fromiter((len(c) for c in chunks), dtype=np.uint64, count=len(chunks))
        offs = np.zeros(len(chunks), dtype=np.uint64)
        if len(chunks) > 1:
            offs[1:] = np.cumsum(lens)[:-1]
        arena = np.frombuffer(b"".join(bytes(c) for c in chunks), dtype=np.uint8)
        self.write_packed(arena, np.asarray(ids, dtype=np.uint64), offs, lens)

    # -- Sum / Reset / state ------------------------------------------------
    def sum(self, ids=None) -> np.ndarray:
        """uint8 [k, 32]: SHA-256 of everything written to each stream (all streams
        for ids=None); no stream changes."""
        ptr, k, keep = self._ids(ids)
        out = np.empty((k, 32), dtype=np.uint8)
        if k:
            self._check(self._lib.msha_streams_sum(self._handle(), ptr, k, _p(out, ctypes.c_uint8)))
        return out

    def reset(self, ids=None) -> None:
        ptr, k, keep = self._ids(ids)
        self._check(self._lib.msha_streams_reset(self._handle(), ptr, k))

    def lengths(self, ids=None) -> np.ndarray:
        """Bytes written to each stream so far."""
        ptr, k, keep = self._ids(ids)
        out = np.zeros(max(k, 1), dtype=np.uint64)
        self._check(self._lib.msha_streams_length(self._handle(), ptr, k, _p(out, ctypes.c_uint64)))
        return out[:k]

    def export_state(self, ids=None) -> np.ndarray:
        """uint8 [k, 108]: each stream's state in the layout of Go crypto/sha256's
        MarshalBinary (that equality is unverified: mirsha.h)."""
        ptr, k, keep = self._ids(ids)
        out = np.zeros((max(k, 1), STATE_BYTES), dtype=np.uint8)
        self._check(self._lib.msha_streams_export(self._handle(), ptr, k, _p(out, ctypes.c_uint8)))
        return out[:k]

    def import_state(self, ids, states) -> None:
        """Streams ids[j] take the exported state states[j] (uint8 [k, 108] or bytes)."""
        if isinstance(states, (bytes, bytearray)):
            states = np.frombuffer(bytes(states), dtype=np.uint8)
        states = np.ascontiguousarray(states, dtype=np.uint8).reshape(-1, STATE_BYTES)
        ptr, k, keep = self._ids(ids)
        if states.shape[0] != k:
            raise ValueError("one %d-byte state per id" % STATE_BYTES)
        sp = states if states.size else np.zeros((1, STATE_BYTES), dtype=np.uint8)
        self._check(self._lib.msha_streams_import(self._handle(), ptr, k, _p(sp, ctypes.c_uint8)))

    def stats(self) -> dict:
        s = L.MshaStreamsStats()
        self._check(self._lib.msha_streams_get_stats(self._handle(), ctypes.byref(s)))
        return {name: getattr(s, name) for name, _ in L.MshaStreamsStats._fields_}

    def stream(self, i: int) -> "StreamView":
        """Stream i as a hash.Hash."""
        if not 0 <= int(i) < self.n:
            raise IndexError(i)
        return StreamView(self, int(i))


class StreamView:
    """One stream of a set with hash.Hash's surface: Write appends, Sum(b) appends
    the digest of everything written so far without resetting."""

    size = 32
    block_size = 64

    def __init__(self, streams: StreamSet, i: int):
        self._set = streams
        self._id = np.array([i], dtype=np.uint64)

    def write(self, p: bytes) -> int:
        self._set.write(self._id, [p])
        return len(p)

    def sum(self, b: bytes = b"") -> bytes:
        return bytes(b) + self._set.sum(self._id)[0].tobytes()

    def reset(self) -> None:
        self._set.reset(self._id)


__all__ = ["StreamSet", "StreamView", "STATE_BYTES"]
