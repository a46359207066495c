"""The boundary matrix of the parts gather (mirbft_amd/csrc/parts_gather.hpp): one batch
of multi-part actions that both tests/test_parts_gather.py (the sanitized host program)
and tests/test_gpu_parts.py (k_digest_parts in one launch) run.

  A. total lengths L = 0..200, each cut at seeded random positions into 0..6 parts,
     empty ones among them;
  B. exhaustively, L in {1, 55, 56, 63, 64, 65, 119, 120, 127, 128} (one byte, and both
     sides of the one-block / two-block padding edges and of the block edges) cut into
     two parts at every position 0..L.

Every part is placed in the arena at a start residue mod 16 of its own -- the residues
cycle, so all 16 occur for first and for second parts -- between filler bytes that
belong to no part: a gather that lets a neighbour's byte through yields another digest.
"""
import hashlib

import numpy as np

EXHAUSTIVE = (1, 55, 56, 63, 64, 65, 119, 120, 127, 128)


class Arena:
    """Parts appended at chosen residues mod 16, random filler in the gaps."""

    def __init__(self, rng):
        self.rng = rng
        self.buf = bytearray()
        self.off, self.len = [], []

    def put(self, data: bytes, residue: int) -> int:
        gap = (residue - len(self.buf)) % 16
        if data and gap == 0 and self.buf:
            gap = 16            # never touching the previous part
        self.buf += self.rng.bytes(gap)
        self.off.append(len(self.buf))
        self.len.append(len(data))
        self.buf += data
        return len(self.off) - 1

    def arrays(self, slack: int = 64):
        arena = np.frombuffer(bytes(self.buf) + self.rng.bytes(slack), dtype=np.uint8)
        return arena, np.array(self.off, dtype=np.uint64), np.array(self.len, dtype=np.uint64)


def boundary_matrix(seed: int = 0x9A27):
    """-> (arena, part_off, part_len, begin, expected digests [n, 32], residues seen)."""
    rng = np.random.default_rng(seed)
    ar = Arena(rng)
    begin, want = [0], []
    tick = [0]

    def residue():
        tick[0] += 1
        return (tick[0] * 5) % 16      # 5 is coprime to 16: every residue, evenly

    def action(pieces):
        for p in pieces:
            ar.put(p, residue())
        begin.append(len(ar.off))
        want.append(hashlib.sha256(b"".join(pieces)).digest())

    for L in range(201):
        msg = rng.bytes(L)
        k = int(rng.integers(0, 7))            # 0..6 parts
        if L == 0:
            k = 0                              # the zero-part action: the empty string
        elif k == 0:
            k = 1
        cuts = sorted(int(c) for c in rng.integers(0, L + 1, size=max(k - 1, 0)))   # equal cuts: empty parts
        edges = [0] + cuts + [L] if k else []
        action([msg[a:b] for a, b in zip(edges, edges[1:])])
    second = 0
    for L in EXHAUSTIVE:
        msg = rng.bytes(L)
        for p in range(L + 1):
            ar.put(msg[:p], residue())
            second += 1
            ar.put(msg[p:], (second * 7 + L) % 16)      # the second part's start residue varied on its own
            begin.append(len(ar.off))
            want.append(hashlib.sha256(msg).digest())
    arena, off, ln = ar.arrays()
    seen = {int(o) % 16 for o, l in zip(off, ln) if l}
    return (arena, off, ln, np.array(begin, dtype=np.uint64),
            np.frombuffer(b"".join(want), dtype=np.uint8).reshape(-1, 32), seen)


def write_batch(path, arena, off, ln, begin):
    """The file tests/cpp/parts_gather_check.cpp reads: little-endian u64 arena_len,
    n_parts, n_actions, then arena, part_off, part_len, action_part_begin."""
    with open(path, "wb") as f:
        f.write(np.array([arena.size, off.size, begin.size - 1], dtype="<u8").tobytes())
        f.write(arena.tobytes())
        f.write(off.astype("<u8").tobytes())
        f.write(ln.astype("<u8").tobytes())
        f.write(begin.astype("<u8").tobytes())
