"""Job lists for msha_dstreams_write_jobs_device (include/mirsha.h "Write jobs in call
order"), shared by tests/test_dstream_jobs_cpu.py (the sanitized host program over
mirbft_amd/csrc/stream_jobs.hpp) and tests/test_gpu_dstream_jobs.py (the kernels).

A case is n streams and k jobs (ids[j], off[j], len[j]) over an arena. Every chunk is
random bytes of its own at a start residue mod 16 that walks through all sixteen, with
filler between chunks that belongs to none, so any reordering, any lost or doubled job
changes a digest. What a case expects comes from numpy and hashlib alone:

  order(case)    numpy.argsort(min(id, n), kind="stable") and the count of valid jobs
  grouped(case)  the host CSR of that order over the touched streams, the form
                 DeviceStreamSet.write_device takes with rows
  digests(case)  hashlib over each touched stream's seed and chunks in job order

The cases (T = the library's tile_jobs):
  order_case()        n = 5, 40 jobs, repeats interleaved across streams, lengths 0..70,
                      streams seeded to tails 0, 1, 55, 63
  pass_edge_case(n)   n in PASS_EDGES: ids 0, n - 1, pairs that differ in exactly one
                      digit, every id at least three times and never twice in a row
  tile_edge_cases(T)  n = 7, k around the wave, the workgroup and the tile
  one_stream_case(T)  n = 3, 4T + 3 jobs all to stream 1, 32-byte chunks, some empty
  distinct_cases()    k = n = 3,000, a random and a reversed permutation
  skew_case()         n = 1,000, k = 20,000, Zipf-like ids, 5 % of them invalid
"""
import hashlib
import struct

import numpy as np

SLACK = 64
PASS_EDGES = ((1, 1), (255, 1), (256, 2), (65535, 2), (65536, 3), (1 << 24, 4))   # n, radix passes
ONE_DIGIT = (0x01, 0x0100, 0x010000, 0x01000000)


def INVALID(n):
    """The ids of dropped jobs: the first two that are not streams, and the largest."""
    return (n, n + 1, (1 << 32) - 1)


class Case:
    def __init__(self, name, n, ids, lens, seed, seeds=None):
        self.name, self.n = name, int(n)
        self.ids = np.asarray(ids, dtype=np.uint32)
        self.len = np.asarray(lens, dtype=np.uint64)
        assert self.ids.size == self.len.size
        rng = np.random.default_rng(seed)
        # chunk j starts at residue (5 j + 3) mod 16, at least one filler byte after the one before
        res = (5 * np.arange(self.ids.size, dtype=np.int64) + 3) % 16
        off = np.zeros(self.ids.size, dtype=np.int64)
        pos = 0
        for j in range(self.ids.size):
            pos += 1
            pos += (int(res[j]) - pos) % 16
            off[j] = pos
            pos += int(self.len[j])
        self.off = off.astype(np.uint64)
        self.arena = rng.integers(0, 256, pos + SLACK, dtype=np.uint8)
        # seeds: {stream: bytes written before the jobs}
        self.seeds = {int(s): rng.bytes(int(t)) for s, t in (seeds or {}).items()}

    @property
    def k(self):
        return int(self.ids.size)

    def chunk(self, j):
        return self.arena[int(self.off[j]): int(self.off[j]) + int(self.len[j])].tobytes()


def order(case):
    """-> (the job order, how many leading jobs are valid): numpy's stable argsort."""
    keys = np.minimum(case.ids.astype(np.uint64), np.uint64(case.n))
    perm = np.argsort(keys, kind="stable").astype(np.uint32)
    return perm, int((keys < case.n).sum())


def grouped(case):
    """-> (rows, part_off, part_len, begin): the valid jobs grouped stably by stream, one
    row per touched stream in ascending order."""
    perm, n_valid = order(case)
    perm = perm[:n_valid]
    keys = case.ids[perm]
    rows, first = np.unique(keys, return_index=True)
    begin = np.append(first, n_valid).astype(np.uint64)
    return rows.astype(np.uint32), case.off[perm], case.len[perm], begin


def seed_batch(case):
    """-> (arena, part_off, part_len, begin, rows) that writes the seeds, or None."""
    if not case.seeds:
        return None
    rows = np.array(sorted(case.seeds), dtype=np.uint32)
    blob, off, ln = bytearray(), [], []
    for s in rows:
        blob += b"\0" * ((3 - len(blob)) % 16 + 16)
        off.append(len(blob))
        ln.append(len(case.seeds[int(s)]))
        blob += case.seeds[int(s)]
    arena = np.frombuffer(bytes(blob) + b"\0" * SLACK, dtype=np.uint8)
    return (arena, np.array(off, dtype=np.uint64), np.array(ln, dtype=np.uint64),
            np.arange(rows.size + 1, dtype=np.uint64), rows)


def digests(case):
    """-> (touched streams ascending, their SHA-256 [m, 32]) by hashlib, fed in job order."""
    h = {}
    for j in range(case.k):
        s = int(case.ids[j])
        if s >= case.n:
            continue
        if s not in h:
            h[s] = hashlib.sha256(case.seeds.get(s, b""))
        h[s].update(case.chunk(j))
    rows = np.array(sorted(h), dtype=np.uint32)
    out = np.frombuffer(b"".join(h[int(s)].digest() for s in rows), dtype=np.uint8).reshape(-1, 32)
    return rows, out


def start_residues(case):
    return {int(o) % 16 for o, ln in zip(case.off, case.len) if ln}


# ---- the cases ---------------------------------------------------------------------
def order_case():
    rng = np.random.default_rng(101)
    ids = np.array([(3 * j + j // 7) % 5 for j in range(40)], dtype=np.uint32)
    lens = rng.integers(0, 71, 40)
    lens[[0, 1, 2, 3]] = (0, 70, 64, 1)
    return Case("order", 5, ids, lens, 102, seeds={0: 64, 1: 1, 2: 55, 3: 63})


def pass_edge_ids(n, distinct=150):
    """About 600 jobs: every chosen id four times or more, never twice in a row (n > 1)."""
    rng = np.random.default_rng(200 + n % 1000)
    want = {0, n - 1}
    for bit in ONE_DIGIT:                       # pairs that differ in exactly one digit
        if bit < n:
            want |= {0, bit}
            base = int(rng.integers(0, n))
            if (base ^ bit) < n:
                want |= {base, base ^ bit}
    while len(want) < min(distinct, n):
        want.add(int(rng.integers(0, n)))
    uniq = np.array(sorted(want), dtype=np.uint32)
    rounds = []
    for _ in range(max(4, -(-4 * distinct // uniq.size))):
        p = rng.permutation(uniq)
        if rounds and uniq.size > 1 and rounds[-1][-1] == p[0]:
            p = np.roll(p, 1)
        rounds.append(p)
    return np.concatenate(rounds)


def pass_edge_case(n):
    ids = pass_edge_ids(n)
    lens = np.random.default_rng(300 + n % 1000).integers(0, 71, ids.size)
    return Case("pass_edge_%d" % n, n, ids, lens, 301 + n % 1000)


def tile_edge_ks(T):
    return (1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 5)


def tile_edge_cases(T):
    out = []
    for k in tile_edge_ks(T):
        rng = np.random.default_rng(400 + k)
        out.append(Case("tile_edge_%d" % k, 7, rng.integers(0, 7, k), rng.integers(0, 41, k), 401 + k))
    return out


def one_stream_case(T):
    k = 4 * T + 3
    lens = np.full(k, 32)
    lens[::11] = 0
    return Case("one_stream", 3, np.full(k, 1), lens, 501, seeds={1: 5})


def distinct_cases():
    rng = np.random.default_rng(600)
    n = 3000
    lens = rng.integers(0, 50, n)
    return [Case("distinct_random", n, rng.permutation(n), lens, 601),
            Case("distinct_reversed", n, np.arange(n)[::-1], lens, 602)]


def skew_case():
    rng = np.random.default_rng(700)
    n, k = 1000, 20000
    ids = np.minimum(rng.zipf(1.3, k) - 1, n - 1).astype(np.uint64)
    ids = (ids * 389) % n                                   # the heavy streams are not neighbours
    bad = rng.random(k) < 0.05
    ids[bad] = rng.choice(np.array(INVALID(n), dtype=np.uint64), int(bad.sum()))
    return Case("skew", n, ids, rng.integers(0, 41, k), 701)


def sort_cases(T):
    """Cases 1-6, as the host program runs them: only n and the ids matter there."""
    return ([order_case()] + [pass_edge_case(n) for n, _ in PASS_EDGES] + tile_edge_cases(T)
            + [one_stream_case(T)] + distinct_cases() + [skew_case()])


def write_ids(path, cases):
    """u64 count, then per case u64 n, u64 k, k x u32 ids (little-endian)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(cases)))
        for c in cases:
            f.write(struct.pack("<QQ", c.n, c.k))
            f.write(c.ids.astype("<u4").tobytes())
