"""Cases and a route model for msha_dstreams_write_routed_device (include/mirsha.h "Device
stream sets: long writes routed to the chain"), shared by tests/test_dstream_route_cpu.py
(the builders proven to reach what they claim, every non-caps case shown to fit both caps)
and tests/test_gpu_dstream_routed.py (the kernels).

The model is written from the header's paragraph alone. A row is LONG when its stream is
below n, its part range is valid and floor((length % 64 + sum of its part lengths) / 64)
>= long_blocks; a long row needs a slot (max_long of them) and room for
round16(length % 64 + sum) bytes while the given bytes plus MSHA_DEVICE_ARENA_SLACK stay
within long_bytes. What the streams hold afterwards is dstream_matrix.Model's business:
routing changes no byte of it.

A case is a `pre` batch that leaves every stream its prior tail (row s of it is stream s),
then the batch under test with its rows and its three opts. Every part sits at a start
residue mod 16 of its own (parts_matrix.Arena).
"""
from dataclasses import dataclass, field

import numpy as np

import parts_matrix

SLACK = 64
MAX_LONG = 64               # explicit in every case: at most 16 x compute units on any gfx950
LONG_BYTES = 1 << 20


def round16(x: int) -> int:
    return (x + 15) // 16 * 16


@dataclass
class Case:
    n: int                          # streams of the set
    tails: list                     # bytes stream s buffers before the call
    pre: tuple                      # the batch that leaves them (row s is stream s)
    batch: tuple                    # arena, part_off, part_len, row_part_begin
    rows: object                    # uint32 array, or None (row r is stream r)
    long_blocks: int
    max_long: int = MAX_LONG
    long_bytes: int = LONG_BYTES
    note: dict = field(default_factory=dict)

    def opts(self):
        return dict(long_blocks=self.long_blocks, max_long=self.max_long, long_bytes=self.long_bytes)


@dataclass
class Route:
    long: set           # rows that are long
    total: dict         # row -> length % 64 + sum, for the long rows
    whole: dict         # row -> blocks its write compresses, for every valid row
    all_fit: bool       # every long row fits both caps: exactly `long` is routed
    count: int          # rows routed (all_fit: len(long); else defined only for long rows of one total)
    invalid_stream: list
    invalid_range: list


def model_of(case: Case, lengths=None) -> Route:
    """lengths: each stream's length before the call (default: the case's tails)."""
    lengths = list(case.tails) if lengths is None else [int(x) for x in lengths]
    arena, off, ln, begin = case.batch
    n_rows = begin.size - 1
    rows = list(range(n_rows)) if case.rows is None else [int(r) for r in case.rows]
    long, total, whole, bad_s, bad_r = set(), {}, {}, [], []
    for r, s in enumerate(rows):
        j0, j1 = int(begin[r]), int(begin[r + 1])
        if s >= case.n:
            bad_s.append(r)
            continue
        if j1 < j0:
            bad_r.append(r)
            continue
        t = lengths[s] % 64
        tot = t + int(ln[j0:j1].sum())
        whole[r] = tot // 64
        if whole[r] >= case.long_blocks:
            long.add(r)
            total[r] = tot
    room = sum(round16(total[r]) for r in long) + SLACK <= case.long_bytes
    all_fit = len(long) <= case.max_long and room
    count = len(long)
    if not all_fit:
        sizes = {total[r] for r in long}
        count = -1
        if len(sizes) == 1:     # the header's formula, for long rows of one total
            (one,) = sizes
            count = min(len(long), case.max_long, max(0, case.long_bytes - SLACK) // round16(one))
    return Route(long, total, whole, all_fit, count, bad_s, bad_r)


def check_route(routed_rows, routed_bytes, route: Route) -> list:
    """What is wrong with a call's routed rows (msha_dstreams_route_read) under the model."""
    out = []
    ids = [int(r) for r in routed_rows]
    if len(set(ids)) != len(ids):
        out.append("a row is routed twice")
    for r in ids:
        if r not in route.long:
            out.append(f"row {r} is routed and is not long")
    if route.all_fit and set(ids) != route.long:
        out.append(f"every long row fits: routed {sorted(ids)} is not long {sorted(route.long)}")
    if not route.all_fit and route.count >= 0 and len(ids) != route.count:
        out.append(f"{len(ids)} rows routed, the header says {route.count}")
    want = sum(round16(route.total[r]) for r in ids if r in route.total)
    if int(routed_bytes) != want:
        out.append(f"routed_bytes {routed_bytes} is not the rounded totals' sum {want}")
    return out


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.pre, self.pre_begin = parts_matrix.Arena(self.rng), [0]
        self.app, self.app_begin = parts_matrix.Arena(self.rng), [0]
        self.tails = []
        self.tick = 0

    def residue(self):
        self.tick += 1
        return (self.tick * 5) % 16

    def stream(self, t):
        """A stream that buffers t bytes before the call."""
        if t:
            self.pre.put(self.rng.bytes(t), self.residue())
        self.pre_begin.append(len(self.pre.off))
        self.tails.append(t)

    def row(self, part_lens, residues=None):
        for k, n in enumerate(part_lens):
            self.app.put(self.rng.bytes(int(n)), self.residue() if residues is None else residues[k])
        self.app_begin.append(len(self.app.off))

    def cut_row(self, total, parts):
        """total bytes cut into `parts` parts at seeded positions (equal cuts: empty parts)."""
        cuts = sorted(int(c) for c in self.rng.integers(0, total + 1, size=parts - 1))
        self.row([b - a for a, b in zip([0] + cuts, cuts + [total])])

    def case(self, long_blocks, rows=None, **kw):
        def batch(ar, begin):
            arena, off, ln = ar.arrays(SLACK)
            return arena, off, ln, np.array(begin, dtype=np.uint64)
        return Case(len(self.tails), list(self.tails), batch(self.pre, self.pre_begin), batch(self.app, self.app_begin),
                    rows, long_blocks, **kw)


EDGE_TAILS = (0, 1, 55, 56, 63)
EDGE_DELTAS = (-1, 0, 1)


def threshold_edge(long_blocks=3):
    """-> (case, combos): row r has prior tail t and t + sum = 64 Lx + d for combos[r] =
    (t, Lx, d), t in EDGE_TAILS, Lx in (long_blocks, long_blocks + 1), d in EDGE_DELTAS."""
    b = _Builder(0x7E01)
    combos = [(t, lx, d) for t in EDGE_TAILS for lx in (long_blocks, long_blocks + 1) for d in EDGE_DELTAS]
    for t, lx, d in combos:
        b.stream(t)
        b.cut_row(64 * lx + d - t, 3)
    return b.case(long_blocks), combos


NEW_TAILS = (0, 1, 15, 16, 17, 63)


def new_tail_edges(long_blocks=2):
    """-> (case, combos): every routed row; (t + sum) % 64 = combos[r][1] in NEW_TAILS for
    prior tails combos[r][0] in (0, 17, 63)."""
    b = _Builder(0x7E02)
    combos = [(t, k) for t in (0, 17, 63) for k in NEW_TAILS]
    for i, (t, k) in enumerate(combos):
        b.stream(t)
        b.cut_row(64 * (long_blocks + i % 2) + k - t, 4)
    return b.case(long_blocks), combos


def gather_paths(long_blocks=4):
    """-> (case, (three, many, short)): row `three` has 3 parts, one of 2,000 bytes at an odd
    offset; row `many` 300 parts of 0..40 bytes, empty ones among them; row `short` stays
    a lane."""
    b = _Builder(0x7E03)
    b.stream(5)
    b.row([7, 2000, 30], residues=[3, 9, 12])
    b.stream(41)
    lens = [int(x) for x in b.rng.integers(0, 41, size=300)]
    for k in range(0, 300, 17):
        lens[k] = 0
    b.row(lens)
    b.stream(9)
    b.row([20, 20])
    return b.case(long_blocks), (0, 1, 2)


def slots(k, long_blocks=2, permute=False, big=False):
    """-> (case, routed): k long rows of 2..5 blocks (big: the first of 65 blocks) between
    short rows, every third row a zero-part row. permute: the rows name a permuted subset
    of a larger set."""
    b = _Builder(0x7E10 + k + (100 if permute else 0) + (200 if big else 0))
    routed, r = [], 0
    for i in range(k):
        b.stream(int(b.rng.integers(0, 64)))        # a short row: under a block in all
        b.cut_row(int(b.rng.integers(1, 64 - b.tails[-1])) if b.tails[-1] < 63 else 0, 2)
        r += 1
        if i % 3 == 0:
            b.stream(int(b.rng.integers(0, 64)))
            b.row([])
            r += 1
        t = int(b.rng.integers(0, 64))
        blocks = 65 if (big and i == 0) else 2 + i % 4
        b.stream(t)
        b.cut_row(64 * blocks + int(b.rng.integers(0, 64)) - t, 1 + i % 5)
        routed.append(r)
        r += 1
    rows = None
    if permute:
        n_rows = len(b.tails)
        extra = 5
        perm = b.rng.permutation(n_rows + extra)[:n_rows].astype(np.uint32)
        # stream perm[r] must hold row r's tail: lay the pre batch out by stream
        tails = [0] * (n_rows + extra)
        for rr, s in enumerate(perm):
            tails[int(s)] = b.tails[rr]
        pre = _Builder(0x7E99 + k)
        for t in tails:
            pre.stream(t)
        b.pre, b.pre_begin, b.tails = pre.pre, pre.pre_begin, tails
        rows = perm
    return b.case(long_blocks, rows=rows), routed


CAP_TAIL = 9
CAP_TOTAL = 1000            # t + sum of each of the five long rows: 15 blocks, round16 = 1008


def caps(max_long, long_bytes):
    """Five long rows of one total CAP_TOTAL among three short ones."""
    b = _Builder(0x7E20)
    for i in range(8):
        if i in (0, 2, 3, 5, 7):
            b.stream(CAP_TAIL)
            b.cut_row(CAP_TOTAL - CAP_TAIL, 3)
        else:
            b.stream(3)
            b.row([10])
    return b.case(4, max_long=max_long, long_bytes=long_bytes)


def errors(long_blocks=2):
    """-> (case, (bad_stream_row, bad_range_row, untouched_stream)): a row naming a stream
    >= n and a row whose part range decreases over parts that would be long, beside
    routed rows and short ones."""
    b = _Builder(0x7E30)
    for t, total in ((3, 300), (60, 20), (17, 700), (5, 400), (0, 40), (33, 200)):
        b.stream(t)
        b.cut_row(total, 2)
    case = b.case(long_blocks)
    arena, off, ln, begin = case.batch
    begin = begin.copy()
    # row 3's range decreases: begin[3] moves past begin[4] (the parts between them hold 700 + 400 bytes)
    begin[3], begin[4] = begin[4] + 0, begin[3] + 0
    # rows: row 2 names a stream out of range
    rows = np.arange(6, dtype=np.uint32)
    rows[2] = case.n + 4
    case.batch = (arena, off, ln, begin)
    case.rows = rows
    return case, (2, 3, 2)


def no_long(long_blocks=4):
    """Every row under the threshold."""
    b = _Builder(0x7E40)
    for i in range(70):
        t = (i * 7) % 64
        b.stream(t)
        b.cut_row(64 * long_blocks - 1 - t if i % 2 else 10 + i, 2)
    return b.case(long_blocks)


def rounds_case(long_blocks=2):
    """A batch of 6 rows, 4 of them long whatever the tails are (>= 3 blocks of parts),
    to be written several times to the same streams."""
    b = _Builder(0x7E50)
    for i, total in enumerate((200, 333, 30, 1001, 0, 4097)):
        b.stream((i * 13) % 64)
        if total:
            b.cut_row(total, 1 + i)
        else:
            b.row([])
    return b.case(long_blocks)
