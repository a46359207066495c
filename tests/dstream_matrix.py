"""Batches and a model for the device stream sets (include/mirsha.h "Device stream sets"),
shared by tests/test_dstream_cpu.py (the sanitized host program over
mirbft_amd/csrc/stream_device.hpp) and tests/test_gpu_dstreams.py (the kernels).

The model is written from the header's paragraph alone: a stream is a hashlib.sha256
fed incrementally, Sum is .copy().digest(), Snap restarts the stream from its sum, a
row that names a stream >= n or whose part range decreases changes nothing. No expected
value comes from the library.

A batch is (arena, part_off, part_len, row_part_begin) as numpy arrays, built on
parts_matrix.Arena: every part sits at a start residue mod 16 of its own between filler
bytes that belong to no part.

  tail_by_append()  for every buffered tail t in 0..63 and every appended total a in
                    0..130 one stream (8,384): a first write leaves t bytes buffered, a
                    second appends a bytes cut into 1..3 parts at seeded positions,
                    empty parts among them. It covers staying under a block, landing
                    exactly on 64 and 128, crossing by one, and the sum's padding edges
                    55 / 56 / 63 / 0 on the length before and after the write.
  three_rounds()    parts_matrix.boundary_matrix()'s batch written three times to the
                    same streams: the tails are whatever the round before left.
"""
import hashlib

import numpy as np

import parts_matrix

SLACK = 64
TAILS = 64
APPENDS = 131


class Model:
    """n streams as the header describes them."""

    def __init__(self, n: int):
        self.n = n
        self.h = [hashlib.sha256() for _ in range(n)]
        self.length = [0] * n
        self.tail = [b""] * n

    def _rows(self, rows, n_rows=None):
        if rows is None:
            assert n_rows is None or n_rows == self.n
            return list(range(self.n))
        return [int(r) for r in rows]

    def write(self, batch, rows=None):
        arena, off, ln, begin = batch
        for r, s in enumerate(self._rows(rows, begin.size - 1)):
            j0, j1 = int(begin[r]), int(begin[r + 1])
            if s >= self.n or j1 < j0:
                continue                                    # flagged: no stream is touched
            for j in range(j0, j1):
                data = arena[int(off[j]): int(off[j]) + int(ln[j])].tobytes()
                self.h[s].update(data)
                self.length[s] += len(data)
                buf = self.tail[s] + data
                keep = self.length[s] % 64
                self.tail[s] = buf[len(buf) - keep:] if keep else b""

    def sum(self, rows=None) -> np.ndarray:
        ids = self._rows(rows)
        out = np.zeros((len(ids), 32), dtype=np.uint8)
        for r, s in enumerate(ids):
            if s < self.n:                                  # out of range: a zero row
                out[r] = np.frombuffer(self.h[s].copy().digest(), dtype=np.uint8)
        return out

    def snap(self, rows=None) -> np.ndarray:
        out = self.sum(rows)
        for r, s in enumerate(self._rows(rows)):
            if s < self.n:
                d = out[r].tobytes()
                self.h[s] = hashlib.sha256(d)
                self.length[s] = 32
                self.tail[s] = d
        return out

    def reset(self, rows=None):
        for s in self._rows(rows):
            if s < self.n:
                self.h[s] = hashlib.sha256()
                self.length[s] = 0
                self.tail[s] = b""

    def lengths(self) -> np.ndarray:
        return np.array(self.length, dtype=np.uint64)

    def buffers(self) -> np.ndarray:
        """uint8 [n, 64]: each stream's buffered bytes, zero past length % 64."""
        out = np.zeros((self.n, 64), dtype=np.uint8)
        for s, t in enumerate(self.tail):
            out[s, :len(t)] = np.frombuffer(t, dtype=np.uint8)
        return out


def _batch(ar, begin):
    arena, off, ln = ar.arrays(SLACK)
    return arena, off, ln, np.array(begin, dtype=np.uint64)


def _cuts(rng, a):
    """a bytes cut into 1..3 parts at seeded positions (equal cuts: empty parts)."""
    k = int(rng.integers(1, 4))
    cuts = sorted(int(c) for c in rng.integers(0, a + 1, size=k - 1))
    return list(zip([0] + cuts, cuts + [a]))


def tail_by_append(seed: int = 0xD57A):
    """-> (pre, app, pairs): stream s = t * 131 + a buffers t bytes after the batch pre
    and appends a bytes with the batch app; pairs[s] = (t, a)."""
    rng = np.random.default_rng(seed)
    pairs = [(t, a) for t in range(TAILS) for a in range(APPENDS)]
    tick = [0]

    def residue():
        tick[0] += 1
        return (tick[0] * 5) % 16

    pre, pre_begin = parts_matrix.Arena(rng), [0]
    for t, _ in pairs:
        if t:                                               # t == 0: a zero-part row
            pre.put(rng.bytes(t), residue())
        pre_begin.append(len(pre.off))
    app, app_begin = parts_matrix.Arena(rng), [0]
    for _, a in pairs:
        data = rng.bytes(a)
        for lo, hi in _cuts(rng, a):
            app.put(data[lo:hi], residue())
        app_begin.append(len(app.off))
    return _batch(pre, pre_begin), _batch(app, app_begin), pairs


def three_rounds():
    """-> (batch, rounds): the boundary matrix's batch, to be written `rounds` times to
    the same streams (one stream per action of the matrix)."""
    arena, off, ln, begin, _, _ = parts_matrix.boundary_matrix()
    return (arena, off, ln, begin), 3


def start_residues(batch) -> set:
    _, off, ln, _ = batch
    return {int(o) % 16 for o, l in zip(off, ln) if l}


def write_rounds(path, n_streams, rounds):
    """The file tests/cpp/stream_device_check.cpp reads. rounds: a list of (batch, rows
    or None, digests uint8 [n_streams, 32] of every stream after the round, lengths).
    Little-endian u64 n_streams, n_rounds; per round arena_len, n_parts, n_rows,
    has_rows, then the arena, part_off, part_len, row_part_begin (n_rows + 1), the rows
    (u32, when has_rows), the digests and the lengths."""
    with open(path, "wb") as f:
        f.write(np.array([n_streams, len(rounds)], dtype="<u8").tobytes())
        for (arena, off, ln, begin), rows, digests, lengths in rounds:
            assert digests.shape == (n_streams, 32) and lengths.size == n_streams
            f.write(np.array([arena.size, off.size, begin.size - 1, 0 if rows is None else 1], dtype="<u8").tobytes())
            f.write(arena.tobytes())
            f.write(off.astype("<u8").tobytes())
            f.write(ln.astype("<u8").tobytes())
            f.write(begin.astype("<u8").tobytes())
            if rows is not None:
                f.write(np.asarray(rows).astype("<u4").tobytes())
            f.write(np.ascontiguousarray(digests).tobytes())
            f.write(np.asarray(lengths).astype("<u8").tobytes())


def model_rounds(n_streams, steps):
    """steps: (batch, rows or None) in order -> the rounds write_rounds() takes, by the model."""
    m = Model(n_streams)
    out = []
    for batch, rows in steps:
        m.write(batch, rows)
        out.append((batch, rows, m.sum(), m.lengths()))
    return out
