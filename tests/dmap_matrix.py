"""The cases and the oracle of the device digest maps (include/mirsha.h "Device digest
maps"), shared by the CPU check (tests/test_dmap_cpu.py, which replays
mirbft_amd/csrc/dmap.hpp under sanitizers) and the GPU test (tests/test_gpu_dmap.py).
HIP-free.

A case is a SEQUENCE of steps on one map: adds, finds and clears. The oracle is a plain
Python dict written from the header's text: key (scope, 32 bytes) -> [id, count], ids given
out in order of first occurrence. It is never the code under test.

A step is small to describe, as in tests/group_matrix.py: slot i holds row
base_rows(val[i]) under scope[i], and a short list of flips then changes one byte each.
The stand-alone check rebuilds the arrays from that description (write_sequences)."""
import os
import re
import struct
from dataclasses import dataclass, field

import numpy as np

from group_matrix import FLIP, SENTINEL, base_rows, capacity  # noqa: F401  (one row generator for both)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "mirbft_amd", "csrc", "dmap.hpp")

NO_ID = 0xFFFFFFFF
ADD, FIND, CLEAR = 0, 1, 2
TILE = 256                      # group::kTile, which dmap::kTile is
RESULT_FIELDS = ("n", "entries", "added", "full", "crossed", "listed", "max_count", "max_id")


def launches():
    """dmap::kLaunches: the kernels of one add."""
    return int(re.search(r"constexpr uint32_t kLaunches = (\d+);", open(HEADER).read()).group(1))


@dataclass
class Step:
    kind: int
    val: object = None                              # np.uint32[n]: the row slot i holds
    scope: object = None                            # np.uint32[n], or None: d_scope NULL
    threshold: int = 0
    crossed_cap: int = 8
    flips: list = field(default_factory=list)       # (slot, byte)
    counts: bool = True                             # add: d_before and d_after given; find: d_count given

    @property
    def n(self):
        return 0 if self.val is None else int(np.asarray(self.val).size)

    def digests(self):
        """-> uint8[32 n]"""
        d = base_rows(self.val).copy()
        for slot, byte in self.flips:
            d[slot, byte] ^= FLIP
        return d.reshape(-1)


def add(val, scope=None, threshold=0, crossed_cap=8, flips=(), counts=True):
    val = np.asarray(val, dtype=np.uint32)
    if scope is not None:
        scope = np.broadcast_to(np.asarray(scope, dtype=np.uint32), val.shape).copy()
    return Step(ADD, val, scope, threshold, crossed_cap, list(flips), counts)


def find(val, scope=None, flips=(), counts=True):
    s = add(val, scope, flips=flips, counts=counts)
    s.kind, s.crossed_cap = FIND, 0
    return s


def clear():
    return Step(CLEAR)


@dataclass
class Sequence:
    name: str
    max_keys: int
    steps: list
    home: object = None                             # MSHA_DMAP_FORCE_HOME, or None
    big: bool = False                               # GPU only: too long for the sanitizer run


# ---------------------------------------------------------------------------------------
# the oracle

def keys_of(digests, scope):
    n = digests.size // 32
    rows = np.asarray(digests, dtype=np.uint8).reshape(n, 32)
    return [(int(scope[i]) if scope is not None else 0, rows[i].tobytes()) for i in range(n)]


class DictMap:
    """The header restated over a dict."""

    def __init__(self, max_keys):
        self.max_keys = max_keys
        self.map = {}                               # key -> [id, count]

    def add(self, digests, scope, threshold, crossed_cap):
        keys = keys_of(digests, scope)
        n = len(keys)
        slots, leader = {}, {}
        for i, k in enumerate(keys):
            slots[k] = slots.get(k, 0) + 1
            leader.setdefault(k, i)
        new = [k for k in leader if k not in self.map]          # dicts keep first occurrence order
        entries_before = len(self.map)
        full = entries_before + len(new) > self.max_keys
        number = {k: entries_before + r for r, k in enumerate(new)}
        ids = np.empty(n, np.uint32)
        before = np.empty(n, np.uint32)
        after = np.empty(n, np.uint32)
        for i, k in enumerate(keys):
            b = self.map[k][1] if k in self.map else 0
            before[i] = b
            after[i] = min(b + slots[k], 0xFFFFFFFF)
            ids[i] = NO_ID if full else (self.map[k][0] if k in self.map else number[k])
        crossed_slot = np.full(crossed_cap, SENTINEL, np.uint32)
        if full:
            return {"ids": ids, "before": before, "after": after, "crossed": crossed_slot,
                    "result": (n, entries_before, len(new), 1, 0, 0, 0, 0)}
        crossing = sorted(i for k, i in leader.items()
                          if threshold > 0 and before[i] < threshold <= after[i])
        listed = min(len(crossing), crossed_cap)
        crossed_slot[:listed] = crossing[:listed]
        best = None
        for k, i in leader.items():
            cand = (int(after[i]), -int(ids[i]))
            best = cand if best is None or cand > best else best
            self.map[k] = [int(ids[i]), int(after[i])]
        return {"ids": ids, "before": before, "after": after, "crossed": crossed_slot,
                "result": (n, len(self.map), len(new), 0, len(crossing), listed, best[0], -best[1])}

    def find(self, digests, scope):
        keys = keys_of(digests, scope)
        ids = np.array([self.map[k][0] if k in self.map else NO_ID for k in keys], np.uint32).reshape(-1)
        count = np.array([self.map[k][1] if k in self.map else 0 for k in keys], np.uint32).reshape(-1)
        return {"ids": ids, "count": count}

    def clear(self):
        self.map = {}

    def state(self):
        """What msha_dmap_read returns for all entries: (scope, digests [entries, 32], count)."""
        by_id = sorted((v[0], k, v[1]) for k, v in self.map.items())
        assert [e[0] for e in by_id] == list(range(len(by_id)))
        scope = np.array([e[1][0] for e in by_id], np.uint32).reshape(-1)
        digests = np.frombuffer(b"".join(e[1][1] for e in by_id), np.uint8).reshape(-1, 32)
        count = np.array([e[2] for e in by_id], np.uint32).reshape(-1)
        return scope, digests, count


def apply(m, step):
    """One step on the oracle: its outputs, and the map's state after it."""
    if step.kind == ADD:
        out = m.add(step.digests(), step.scope, step.threshold, step.crossed_cap)
        if not step.counts:
            out["before"] = out["after"] = None
    elif step.kind == FIND:
        out = m.find(step.digests(), step.scope)
        if not step.counts:
            out["count"] = None
    else:
        m.clear()
        out = {}
    out["kind"] = step.kind
    out["state"] = m.state()
    return out


def run_oracle(seq):
    m = DictMap(seq.max_keys)
    return [apply(m, s) for s in seq.steps]


def problems(want, got):
    """What differs between two step results (of apply's shape). An array that the step
    was not given (None in want) is not looked at."""
    out = []
    if want["kind"] != got["kind"]:
        return ["kind differs"]
    for name in ("ids", "before", "after", "count", "crossed"):
        w = want.get(name)
        if w is None:
            continue
        g = got.get(name)
        if g is None or len(g) != len(w):
            out.append("%s is missing or of another length" % name)
        elif not np.array_equal(np.asarray(w, np.uint32), np.asarray(g, np.uint32)):
            k = int(np.flatnonzero(np.asarray(w, np.uint32) != np.asarray(g, np.uint32))[0])
            out.append("%s differs at %d: expected %d, got %d" % (name, k, w[k], g[k]))
    if "result" in want and tuple(want["result"]) != tuple(got.get("result", ())):
        out.append("result: expected %s, got %s" % (dict(zip(RESULT_FIELDS, want["result"])), got.get("result")))
    for name, w, g in zip(("state scope", "state digests", "state count"), want["state"], got["state"]):
        if w.shape != np.asarray(g).shape:
            out.append("%s: %d entries expected, got %d" % (name, w.shape[0], np.asarray(g).shape[0]))
        elif not np.array_equal(w, g):
            out.append("%s differs" % name)
    return out


# ---------------------------------------------------------------------------------------
# the sequences

def sizes():
    """The wave (64) and tile (256) edges, and one past two tiles."""
    return [1, 63, 64, 65, 255, 256, 257, 513]


def patterns(n):
    rng = np.random.default_rng(0xD3A9 + n)
    return {"distinct": np.arange(n, dtype=np.uint32) + 1000,
            "equal": np.full(n, 77, dtype=np.uint32),
            "random": rng.integers(0, max(1, n // 4), n).astype(np.uint32)}


def one_call_sequences():
    """One add on an empty map; all distinct fits exactly. A find of the same slots after it."""
    out = []
    for n in sizes():
        for name, val in patterns(n).items():
            keys = int(np.unique(val).size)
            out.append(Sequence("one_%d_%s" % (n, name), keys, [add(val, threshold=2), find(val)]))
    return out


BIG = 65537                     # 257 tiles: k_dmap_scan takes a second chunk of 256


def big_sequence():
    return Sequence("big_exact_fit", BIG, [add(np.arange(BIG, dtype=np.uint32), threshold=1, crossed_cap=4)], big=True)


def across_sequences():
    a = np.arange(300, dtype=np.uint32)
    evens = (2 * np.arange(300)).astype(np.uint32)                 # 0, 2 .. 598
    mixed = np.arange(700, dtype=np.uint32)                        # evens below 600 are held, the rest is new
    far = np.arange(300, dtype=np.uint32) + 5000
    far[280] = far[290] = far[5]                                   # leader in tile 0, two members in tile 1
    return [
        Sequence("twice", 300, [add(a, threshold=2), add(a, threshold=2), add(a[::-1].copy(), threshold=3)]),
        Sequence("disjoint", 700, [add(a), add(a + 300), find(np.arange(700, dtype=np.uint32))]),
        Sequence("interleaved", 1000, [add(evens), add(mixed, threshold=2, crossed_cap=400), find(mixed)]),
        Sequence("leader_elsewhere", 400, [add(far, threshold=3), add(far, threshold=4)]),
        Sequence("scoped", 64, [add(np.full(96, 9, np.uint32), scope=np.arange(96) % 3),
                                add(np.full(4, 9, np.uint32), scope=np.array([2, 3, 1 << 31, 0])),
                                find(np.full(3, 9, np.uint32)), find(np.full(3, 9, np.uint32), scope=[0, 5, 1 << 31])]),
    ]


def stored_compare_sequences():
    """A second call's key differs from STORED key 3 in one byte only (each of the 32), or
    in the scope only: it becomes entry 65, and the map's key 3 and key 10 are found."""
    base = np.arange(65, dtype=np.uint32)
    second = np.array([3, 3, 10], dtype=np.uint32)
    out = [Sequence("stored_byte_%d" % b, 80, [add(base, scope=7), add(second, scope=7, flips=[(0, b)], threshold=2)])
           for b in range(32)]
    out.append(Sequence("stored_scope", 80, [add(base, scope=7),
                                             add(second, scope=np.array([7 | 1 << 31, 7, 7]), threshold=2)]))
    return out


def probe_sequences():
    """max_keys 8: capacity 64. Every key at one home, 0 and then 63 (the chain wraps
    around): three adds that fill the map exactly, a find after each."""
    steps = [add([1, 2, 3, 2]), find([3, 2, 1, 4]),
             add([9, 2, 8, 9]), find([8, 9, 1, 2, 3, 7]),
             add([5, 6, 1, 7, 5]), find(np.arange(12))]
    return [Sequence("chain_home_%d" % h, 8, steps, home=h) for h in (0, 63)]


def full_sequence():
    return Sequence("full", 4, [
        add([1, 2, 3, 1], threshold=2),
        add([8, 2, 9, 2], threshold=1),          # two new and one held: refused whole
        find([1, 2, 3, 8, 9]),
        add([8, 2], threshold=3),                # one new: id 3
        add([9]),                                # one more: refused
        add([2, 2, 8]),                          # held keys alone still go in
        find([9, 8])])


def crossing_sequences():
    A, B, C, D = 11, 12, 13, 14
    wide = np.arange(600, dtype=np.uint32) + 100
    wide[[10, 11, 12]] = 50                      # a crossing leader in tile 0 ...
    wide[[300, 301, 302]] = 51                   # ... and one in tile 1
    five = np.repeat(np.arange(5, dtype=np.uint32) + 20, 3)
    return [
        Sequence("crossing", 16, [add([A, B, A, C, C, D, A, B, C], threshold=3),         # A 0->3, C 0->3 listed
                                  add([D, C, B, C], threshold=3),                       # B 2->3 listed; C 3->5, D 1->2 not
                                  add([A, B, C, D, D], threshold=0),                    # no threshold: crossed 0
                                  add([B, B, B, B], threshold=7, crossed_cap=0),        # a NULL list
                                  add([B], threshold=9, crossed_cap=0)]),
        Sequence("crossing_cap", 16, [add(five, threshold=3, crossed_cap=2), add(five, threshold=6, crossed_cap=5)]),
        Sequence("crossing_two_tiles", 600, [add(wide, threshold=3, crossed_cap=4)]),
    ]


def other_sequences():
    a = np.arange(70, dtype=np.uint32) % 9
    return [
        Sequence("no_counts", 16, [add(a, threshold=5, counts=False), add(a, threshold=10, counts=False),
                                   find(a, counts=False)]),
        Sequence("clear_reuse", 16, [add(a), clear(), find(a), add([4, 100, 3, 4], threshold=2), clear(), clear(),
                                     add([7])]),
        Sequence("find", 16, [find([1, 2]), add([1, 2, 1]), find([2, 5, 1, 1, 6]), find([5], counts=False)]),
    ]


def all_sequences():
    return (one_call_sequences() + [big_sequence()] + across_sequences() + stored_compare_sequences() +
            probe_sequences() + [full_sequence()] + crossing_sequences() + other_sequences())


# ---------------------------------------------------------------------------------------
# the stand-alone check's files

def _words(a):
    b = np.ascontiguousarray(a).tobytes()
    return b + b"\0" * (-len(b) % 8)


def write_sequences(path, seqs):
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(seqs)))
        for s in seqs:
            f.write(struct.pack("<3q", s.max_keys, -1 if s.home is None else s.home, len(s.steps)))
            for st in s.steps:
                f.write(struct.pack("<7q", st.kind, st.n, int(st.scope is not None), st.threshold, st.crossed_cap,
                                    len(st.flips), int(st.counts)))
                if st.kind == CLEAR:
                    continue
                f.write(_words(np.asarray(st.val, dtype="<u4")))
                if st.scope is not None:
                    f.write(_words(np.asarray(st.scope, dtype="<u4")))
                f.write(_words(np.asarray(st.flips, dtype="<u4").reshape(-1)))


def read_results(path, seqs):
    """-> per sequence, per step, a result of apply's shape."""
    data = open(path, "rb").read()
    at = 0

    def take(dtype, count):
        nonlocal at
        size = np.dtype(dtype).itemsize * count
        a = np.frombuffer(data, dtype=dtype, count=count, offset=at).copy()
        at += size + (-size % 8)
        return a

    out = []
    for s in seqs:
        steps = []
        for st in s.steps:
            r = {"kind": st.kind}
            if st.kind == ADD:
                r["result"] = tuple(int(x) for x in take("<u8", 8))
                r["ids"] = take("<u4", st.n)
                before, after = take("<u4", st.n), take("<u4", st.n)
                r["before"], r["after"] = (before, after) if st.counts else (None, None)
                r["crossed"] = take("<u4", st.crossed_cap)
            elif st.kind == FIND:
                r["ids"] = take("<u4", st.n)
                count = take("<u4", st.n)
                r["count"] = count if st.counts else None
            entries = int(take("<u8", 1)[0])
            r["state"] = (take("<u4", entries), take("u1", 32 * entries).reshape(-1, 32), take("<u4", entries))
            steps.append(r)
        out.append(steps)
    assert at == len(data)
    return out
