"""Cases for msha_dstreams_write_jobs_routed_device (include/mirsha.h "Device stream sets:
jobs in call order with the long streams routed to the chain"), shared by
tests/test_dstream_jobs_route_cpu.py (the builders proven to reach what they claim, every
non-caps case shown to fit both caps) and tests/test_gpu_dstream_jobs_routed.py.

A case is jobs in call order (stream, offset, length) over an arena, a `pre` batch that
leaves every stream its prior tail (row s of it is stream s) and the three opts. Nothing
here models the entry anew: stable grouping of the jobs by stream (grouped()) gives a
case of tests/dstream_route_matrix.py whose row r is stream streams[r], so that module's
route model (model_of, check_route) and the stream model (dstream_matrix.Model) apply
unchanged -- "row" read as "stream", "its parts" as "its valid jobs", as the header says.

The core is jobs_of(route_case, interleave): row r's parts become jobs of stream rows[r]
(or r), dealt in one of three orders that all keep a row's own order
  "round_robin"  one job of every row in turn
  "reversed"     the rows last to first, each row's jobs contiguous
  "shuffle"      a seeded shuffle of the rows' turns
Jobs-only builders cover what a CSR cannot say: dropped jobs, empty chunks, the radix
passes' top digits, the sort's tile boundary, and the reference's shape made small.
"""
import struct
from dataclasses import dataclass, field

import numpy as np

import dstream_jobs_matrix as J
import dstream_route_matrix as M
import parts_matrix
import stream_matrix as S

SLACK = M.SLACK
INTERLEAVES = ("round_robin", "reversed", "shuffle")
STATE_BYTES = 108


@dataclass
class JobCase:
    n: int                          # streams of the set
    tails: dict                     # stream -> bytes it buffers before the call (absent: 0)
    pre: object                     # the batch that leaves them (row s is stream s), or None
    arena: np.ndarray
    ids: np.ndarray                 # uint32, the jobs' streams in call order
    off: np.ndarray                 # uint64
    len: np.ndarray                 # uint64
    long_blocks: int
    max_long: int = M.MAX_LONG
    long_bytes: int = M.LONG_BYTES
    defaults: bool = False          # the call passes no opts: the three above are what the model assumes
    note: dict = field(default_factory=dict)

    @property
    def k(self):
        return int(self.ids.size)

    def opts(self):
        if self.defaults:
            return {}
        return dict(long_blocks=self.long_blocks, max_long=self.max_long, long_bytes=self.long_bytes)

    def valid(self):
        return self.ids.astype(np.uint64) < np.uint64(self.n)

    def touched(self):
        """The streams some valid job names, ascending."""
        return np.unique(self.ids[self.valid()]).astype(np.uint32)

    def chunk(self, j):
        return self.arena[int(self.off[j]): int(self.off[j]) + int(self.len[j])].tobytes()


def order(case):
    """-> (the job order, how many leading jobs are valid): numpy's stable argsort of min(id, n)."""
    keys = np.minimum(case.ids.astype(np.uint64), np.uint64(case.n))
    return np.argsort(keys, kind="stable").astype(np.uint32), int((keys < case.n).sum())


def grouped(case, streams=None):
    """-> (streams, route case): the valid jobs grouped stably by stream as a case of
    dstream_route_matrix whose row r is stream streams[r] (ascending; default: all n),
    rows None, n = len(streams). Every valid job's stream must be among them. A large
    set's case is modelled over its touched streams alone: a stream's route depends on
    its own tail and jobs only."""
    streams = np.arange(case.n, dtype=np.uint32) if streams is None else np.asarray(streams, dtype=np.uint32)
    assert np.all(streams[1:] > streams[:-1]) and (streams.size == 0 or int(streams[-1]) < case.n)
    perm, n_valid = order(case)
    perm = perm[:n_valid]
    keys = case.ids[perm]
    assert np.isin(keys, streams).all()
    begin = np.searchsorted(keys, np.append(streams, np.uint32(0xFFFFFFFF)), side="left").astype(np.uint64)
    begin[-1] = n_valid
    tails = [int(case.tails.get(int(s), 0)) for s in streams]
    rc = M.Case(int(streams.size), tails, case.pre, (case.arena, case.off[perm], case.len[perm], begin), None,
                case.long_blocks, max_long=case.max_long, long_bytes=case.long_bytes)
    return streams, rc


def stream_bytes(case):
    """{stream: the bytes its valid jobs append, in job order}, restated from the jobs alone."""
    out = {}
    for j in range(case.k):
        s = int(case.ids[j])
        if s < case.n:
            out[s] = out.get(s, b"") + case.chunk(j)
    return out


def row_bytes(route_case):
    """{stream: the bytes its row appends} of a dstream_route_matrix case with valid rows."""
    arena, off, ln, begin = route_case.batch
    out = {}
    for r in range(begin.size - 1):
        s = r if route_case.rows is None else int(route_case.rows[r])
        out[s] = b"".join(arena[int(off[j]): int(off[j]) + int(ln[j])].tobytes()
                          for j in range(int(begin[r]), int(begin[r + 1])))
    return out


def _turns(counts, interleave, seed):
    """The rows' turns: a sequence of row indices holding row r counts[r] times."""
    rows = range(len(counts))
    if interleave == "round_robin":
        return [r for i in range(max(counts, default=0)) for r in rows if i < counts[r]]
    if interleave == "reversed":
        return [r for r in reversed(rows) for _ in range(counts[r])]
    assert interleave == "shuffle"
    turns = np.array([r for r in rows for _ in range(counts[r])], dtype=np.int64)
    np.random.default_rng(seed).shuffle(turns)
    return [int(r) for r in turns]


def jobs_of(route_case, interleave, seed=0x10B5):
    """A dstream_route_matrix case (every row valid) as jobs: row r's parts, in the row's
    order, are jobs of stream rows[r] (or r), the rows' turns dealt as `interleave` says."""
    arena, off, ln, begin = route_case.batch
    n_rows = begin.size - 1
    stream = list(range(n_rows)) if route_case.rows is None else [int(s) for s in route_case.rows]
    counts = [int(begin[r + 1]) - int(begin[r]) for r in range(n_rows)]
    nxt = [int(begin[r]) for r in range(n_rows)]
    ids, parts = [], []
    for r in _turns(counts, interleave, seed):
        ids.append(stream[r])
        parts.append(nxt[r])
        nxt[r] += 1
    parts = np.array(parts, dtype=np.int64)
    tails = {s: int(t) for s, t in enumerate(route_case.tails) if t}
    return JobCase(route_case.n, tails, route_case.pre, arena, np.array(ids, dtype=np.uint32),
                   off[parts] if parts.size else off[:0], ln[parts] if parts.size else ln[:0],
                   route_case.long_blocks, max_long=route_case.max_long, long_bytes=route_case.long_bytes,
                   note={"interleave": interleave})


def converted():
    """[(name, route case, caps?)]: the cases of dstream_route_matrix the converter runs over."""
    out = [("threshold_edge_%d" % lb, M.threshold_edge(lb)[0], False) for lb in (2, 3, 4)]
    out.append(("new_tail_edges", M.new_tail_edges()[0], False))
    out.append(("gather_paths", M.gather_paths()[0], False))
    for k in (1, 8, 9, 16, 17):
        out.append(("slots_%d" % k, M.slots(k)[0], False))
        out.append(("slots_%d_permuted" % k, M.slots(k, permute=True)[0], False))
    for max_long, long_bytes in CAPS:
        out.append(("caps_%d_%d" % (max_long, long_bytes), M.caps(max_long, long_bytes), True))
    out.append(("no_long", M.no_long(), False))
    out.append(("rounds_case", M.rounds_case(), False))
    return out


R16 = M.round16(M.CAP_TOTAL)
CAPS = ((1, M.LONG_BYTES), (2, M.LONG_BYTES), (5, M.LONG_BYTES), (64, 5 * R16 + SLACK), (64, 5 * R16 + SLACK - 1),
        (64, 3 * R16 + SLACK), (64, 3 * R16 + SLACK - 1))
CAPS_WANT = (1, 2, 5, 5, 4, 3, 2)


# ---- jobs-only builders ------------------------------------------------------------
class _Jobs:
    """Jobs appended in call order, every chunk random bytes at a start residue of its
    own; streams given prior tails by a pre batch over streams 0 .. n - 1."""

    def __init__(self, seed, n, tails=None):
        self.rng = np.random.default_rng(seed)
        self.n = n
        self.ar = parts_matrix.Arena(self.rng)
        self.ids = []
        self.tick = 0
        self.tails = {int(s): int(t) for s, t in (tails or {}).items() if t}
        self.pre = None
        if self.tails:
            pre, begin = parts_matrix.Arena(self.rng), [0]
            for s in range(n):
                if self.tails.get(s):
                    pre.put(self.rng.bytes(self.tails[s]), self.residue())
                begin.append(len(pre.off))
            arena, off, ln = pre.arrays(SLACK)
            self.pre = (arena, off, ln, np.array(begin, dtype=np.uint64))

    def residue(self):
        self.tick += 1
        return (self.tick * 5) % 16

    def job(self, stream, nbytes):
        self.ar.put(self.rng.bytes(int(nbytes)), self.residue())
        self.ids.append(int(stream))

    def deal(self, lists):
        """lists: [(stream, [lengths])]; one job of each in turn, every list in its own order."""
        for r in _turns([len(x) for _, x in lists], "round_robin", 0):
            s, lens = lists[r]
            self.job(s, lens.pop(0))

    def case(self, long_blocks, **kw):
        arena, off, ln = self.ar.arrays(SLACK)
        return JobCase(self.n, dict(self.tails), self.pre, arena, np.array(self.ids, dtype=np.uint32), off, ln,
                       long_blocks, **kw)


def _cut(rng, total, parts):
    cuts = sorted(int(c) for c in rng.integers(0, total + 1, size=parts - 1))
    return [b - a for a, b in zip([0] + cuts, cuts + [total])]


DROP_LEN = 40


def dropped_jobs(long_blocks=3):
    """-> (case, (below, at, short)): ids n, n + 1 and 0xFFFFFFFF dealt between the jobs of
    stream `below`, one byte under the threshold, which the dropped jobs' DROP_LEN bytes
    each would carry over (note["adopt"]: the stream a naive count would give them to),
    and of stream `at`, at the threshold exactly; the call's last job is dropped."""
    n = 4
    b = _Jobs(0x7F01, n, tails={0: 5, 1: 0, 2: 9, 3: 3})
    below, at, short = 0, 1, 2
    bad = list(J.INVALID(n))
    b.deal([(below, _cut(b.rng, 64 * long_blocks - 1 - 5, 6)), (bad[0], [DROP_LEN, DROP_LEN]),
            (at, _cut(b.rng, 64 * long_blocks, 5)), (bad[1], [DROP_LEN]), (short, [20, 20]), (bad[2], [DROP_LEN, DROP_LEN])])
    b.job(bad[1], DROP_LEN)
    case = b.case(long_blocks)
    case.note = {"adopt": {j: below for j in range(case.k) if int(case.ids[j]) >= n}}
    return case, (below, at, short)


def empty_chunks(long_blocks=2):
    """-> (case, names): names = dict of streams -- `inside` long with empty chunks among
    its jobs, `only_empty` with nothing but empty chunks (it keeps its tail), `one_job`
    long in a single job, `wave_below` and `wave_at` long in kWaveSumParts - 1 and
    kWaveSumParts jobs (a lane sums the one, its wave the other), `large` long in a single
    chunk of kLargePart bytes (the whole workgroup copies it)."""
    wave, large = 32, 512
    names = dict(inside=0, only_empty=1, one_job=2, wave_below=3, wave_at=4, large=5)
    b = _Jobs(0x7F02, 6, tails={0: 11, 1: 7, 2: 63, 3: 0, 4: 1, 5: 17})
    b.deal([(0, [40, 0, 50, 0, 0, 60, 0, 33]), (1, [0] * 5), (2, [200]),
            (3, _cut(b.rng, 400, wave - 1)), (4, _cut(b.rng, 400, wave)), (5, [large])])
    case = b.case(long_blocks)
    case.note = {"wave": wave, "large": large}
    return case, names


PASS_LONG_IDS = (0, 255, 256, 65535)


def pass_edges(n, long_blocks=2):
    """-> (case, long streams): a set of n streams (n in dstream_jobs_matrix.PASS_EDGES);
    the long streams sit at the ids that differ only in the top digit of each radix pass --
    0, 255, 256, 65,535 and n - 1, as far as they are below n -- between the short jobs of
    pass_edge_ids(n). No stream has a prior tail."""
    long_ids = sorted({s for s in PASS_LONG_IDS if s < n} | {n - 1})
    b = _Jobs(0x7F10 + n % 1000, n)
    short_ids = [int(s) for s in J.pass_edge_ids(n, distinct=40) if int(s) not in long_ids]
    lists = [(s, _cut(b.rng, 64 * (long_blocks + i % 3) + 7 * i, 5 + i)) for i, s in enumerate(long_ids)]
    turn = 0                                              # a job of each long stream, then eight short ones
    while any(lens for _, lens in lists) or short_ids:
        for s, lens in lists:
            if lens:
                b.job(s, lens.pop(0))
        for _ in range(8):
            if short_ids:
                b.job(short_ids.pop(0), 1 + turn % 7)     # under 64 bytes a short stream in all: see the CPU test
                turn += 1
    return b.case(long_blocks), long_ids


def tile_edges(T, k):
    """-> (case, long stream): n = 7 and k jobs, k around the sort's tile of T jobs; the one
    long stream's jobs sit at the call's first and last positions and on both sides of
    position T (as far as k reaches); the other six streams take 0..3 bytes a job and
    stay far under the default threshold, which this case runs with."""
    n, long_stream = 7, 3
    want = {0, 1, k - 2, k - 1} | {p for p in (T - 2, T - 1, T, T + 1) if p < k}
    b = _Jobs(0x7F20 + k % 1000, n)
    others = [s for s in range(n) if s != long_stream]
    for p in range(k):
        if p in want:
            b.job(long_stream, 1024)
        else:
            b.job(others[(p * 5 + p // 11) % len(others)], p % 4)
    case = b.case(64)                  # MSHA_DSTREAMS_ROUTE_LONG_BLOCKS_DEFAULT, given explicitly
    case.note = {"positions": sorted(want)}
    return case, long_stream


def reference_shape(n=4, digests=512):
    """NodeState.Apply's shape made small: digest d of 32 bytes goes to every node before
    the next, job j to stream j % n, and the call passes no opts. Each stream takes
    digests / 2 blocks, so with the default threshold of 64 all n are routed."""
    rng = np.random.default_rng(0x7F30)
    k = n * digests
    arena = rng.integers(0, 256, 32 * k + SLACK, dtype=np.uint8)
    return JobCase(n, {}, None, arena, (np.arange(k) % n).astype(np.uint32), 32 * np.arange(k, dtype=np.uint64),
                   np.full(k, 32, dtype=np.uint64), 64, defaults=True)


# ---- what the GPU test compares the exports with -------------------------------------
class Fed:
    """The bytes each of some streams was fed, to restate its exported state in Python:
    FIPS 180-4 for the chaining state (stream_matrix), the rest by hand."""

    def __init__(self, streams):
        self.streams = [int(s) for s in streams]
        self.data = {s: b"" for s in self.streams}

    def write(self, batch, rows=None):
        arena, off, ln, begin = batch
        ids = range(begin.size - 1) if rows is None else [int(r) for r in rows]
        for r, s in enumerate(ids):
            if s in self.data:
                self.data[s] += b"".join(arena[int(off[j]): int(off[j]) + int(ln[j])].tobytes()
                                         for j in range(int(begin[r]), int(begin[r + 1])))

    def write_jobs(self, case):
        for s, d in stream_bytes(case).items():
            self.data[s] += d

    def export(self):
        out = np.zeros((len(self.streams), STATE_BYTES), dtype=np.uint8)
        for i, s in enumerate(self.streams):
            d = self.data[s]
            keep = len(d) % 64
            row = (b"sha\x03" + struct.pack(">8I", *S.midstate(d)) + (d[len(d) - keep:] if keep else b"").ljust(64, b"\0")
                   + struct.pack(">Q", len(d)))
            out[i] = np.frombuffer(row, dtype=np.uint8)
        return out
