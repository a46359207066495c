"""The cases and the oracle of the vote maps (include/mirsha.h "Device digest maps that
count voters"), shared by the CPU check (tests/test_dmap_vote_cpu.py, which replays
mirbft_amd/csrc/dmap_vote.hpp under sanitizers) and the GPU test
(tests/test_gpu_dmap_votes.py). HIP-free.

A case is a SEQUENCE of steps on one vote map: votes, find_votes and clears, described as
in tests/dmap_matrix.py (whose step and sequence machinery and row generator are used as
they stand) plus one voter a slot. The oracle is a plain Python dict written from the
header's text: key (scope, 32 bytes) -> [id, set of voters]. It is never the code under
test."""
import os
import re
import struct
from dataclasses import dataclass

import numpy as np

import dmap_matrix as M
from dmap_matrix import CLEAR, NO_ID, SENTINEL, TILE, capacity, clear, keys_of  # noqa: F401

ROOT = M.ROOT
HEADER = os.path.join(ROOT, "mirbft_amd", "csrc", "dmap_vote.hpp")

VOTE, FIND_VOTES = 3, 4
RESULT_FIELDS = M.RESULT_FIELDS + ("counted", "repeats", "bad_voters")
ALL32 = 0xFFFFFFFF


def launches():
    """dmap_vote::kLaunches: the kernels of one vote."""
    return int(re.search(r"constexpr uint32_t kLaunches = (\d+);", open(HEADER).read()).group(1))


def words(max_voters):
    return (max_voters + 31) // 32


@dataclass
class VStep(M.Step):
    voter: object = None                            # np.uint32[n]: the sender of slot i


def vote(val, voter, scope=None, threshold=0, crossed_cap=8, flips=(), counts=True):
    s = M.add(val, scope, threshold, crossed_cap, flips, counts)
    voter = np.broadcast_to(np.asarray(voter, dtype=np.uint32), s.val.shape).copy()
    return VStep(VOTE, s.val, s.scope, threshold, crossed_cap, list(flips), counts, voter)


def find_votes(val, voter, scope=None, flips=(), counts=True):
    s = vote(val, voter, scope, flips=flips, counts=counts)
    s.kind, s.crossed_cap = FIND_VOTES, 0
    return s


@dataclass
class VSequence(M.Sequence):
    max_voters: int = 4
    pair_home: object = None                        # MSHA_DMAP_PAIR_FORCE_HOME, or None


# ---------------------------------------------------------------------------------------
# the oracle

class VoteMap:
    """The header restated over a dict of sets."""

    def __init__(self, max_keys, max_voters):
        self.max_keys, self.max_voters = max_keys, max_voters
        self.map = {}                               # key -> [id, set(voters)]

    def vote(self, digests, scope, voter, threshold, crossed_cap):
        keys = keys_of(digests, scope)
        n = len(keys)
        leader = {}
        for i, k in enumerate(keys):
            leader.setdefault(k, i)
        new = [k for k in leader if k not in self.map]
        entries_before = len(self.map)
        full = entries_before + len(new) > self.max_keys
        number = {k: entries_before + r for r, k in enumerate(new)}
        counted = np.zeros(n, np.uint32)
        fresh, seen = {k: set() for k in leader}, set()
        bad = 0
        for i, k in enumerate(keys):
            v = int(voter[i])
            if v >= self.max_voters:                                        # (a)
                bad += 1
                continue
            if (k, v) in seen:                                              # (b): a smaller slot has it
                continue
            seen.add((k, v))
            if k in self.map and v in self.map[k][1]:                       # (c): voted before the call
                continue
            counted[i] = 1
            fresh[k].add(v)
        ids, before, after = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.uint32)
        for i, k in enumerate(keys):
            b = len(self.map[k][1]) if k in self.map else 0
            before[i], after[i] = b, b + len(fresh[k])
            ids[i] = NO_ID if full else (self.map[k][0] if k in self.map else number[k])
        n_counted = int(counted.sum())
        tail = (n_counted, n - bad - n_counted, bad)
        crossed_slot = np.full(crossed_cap, SENTINEL, np.uint32)
        out = {"ids": ids, "counted": counted, "before": before, "after": after, "crossed": crossed_slot}
        if full:
            out["result"] = (n, entries_before, len(new), 1, 0, 0, 0, 0) + tail
            return out
        crossing = sorted(i for k, i in leader.items() if threshold > 0 and before[i] < threshold <= after[i])
        listed = min(len(crossing), crossed_cap)
        crossed_slot[:listed] = crossing[:listed]
        best = None
        for k, i in leader.items():
            cand = (int(after[i]), -int(ids[i]))
            best = cand if best is None or cand > best else best
            if k not in self.map:
                self.map[k] = [int(ids[i]), set()]
            self.map[k][1] |= fresh[k]
        out["result"] = (n, len(self.map), len(new), 0, len(crossing), listed, best[0], -best[1]) + tail
        return out

    def find_votes(self, digests, scope, voter):
        keys = keys_of(digests, scope)
        held = [self.map.get(k) for k in keys]
        return {"ids": np.array([h[0] if h else NO_ID for h in held], np.uint32).reshape(-1),
                "count": np.array([len(h[1]) if h else 0 for h in held], np.uint32).reshape(-1),
                "voted": np.array([1 if h and int(v) in h[1] else 0 for h, v in zip(held, voter)], np.uint32).reshape(-1)}

    def clear(self):
        self.map = {}

    def state(self):
        """What msha_dmap_read and msha_dmap_read_voters return for all entries: (scope,
        digests [entries, 32], count, masks [entries, words])."""
        by_id = sorted((v[0], k, v[1]) for k, v in self.map.items())
        assert [e[0] for e in by_id] == list(range(len(by_id)))
        scope = np.array([e[1][0] for e in by_id], np.uint32).reshape(-1)
        digests = np.frombuffer(b"".join(e[1][1] for e in by_id), np.uint8).reshape(-1, 32)
        count = np.array([len(e[2]) for e in by_id], np.uint32).reshape(-1)
        masks = np.zeros((len(by_id), words(self.max_voters)), np.uint32)
        for row, e in enumerate(by_id):
            for v in e[2]:
                masks[row, v // 32] |= np.uint32(1 << (v % 32))
        return scope, digests, count, masks


def apply(m, step):
    """One step on the oracle: its outputs, and the map's state after it."""
    if step.kind == VOTE:
        out = m.vote(step.digests(), step.scope, step.voter, step.threshold, step.crossed_cap)
        if not step.counts:
            out["before"] = out["after"] = out["counted"] = None
    elif step.kind == FIND_VOTES:
        out = m.find_votes(step.digests(), step.scope, step.voter)
        if not step.counts:
            out["count"] = None
    else:
        m.clear()
        out = {}
    out["kind"] = step.kind
    out["state"] = m.state()
    return out


def run_oracle(seq):
    m = VoteMap(seq.max_keys, seq.max_voters)
    return [apply(m, s) for s in seq.steps]


def popcount(masks):
    m = np.asarray(masks, np.uint32)
    if m.size == 0:
        return np.zeros(m.shape[0], np.uint32)
    return np.unpackbits(np.ascontiguousarray(m).view(np.uint8).reshape(m.shape[0], -1), axis=1).sum(axis=1).astype(np.uint32)


def problems(want, got):
    """dmap_matrix.problems (ids, before, after, count, crossed, the result, read's three
    arrays) extended with counted, voted, the eleven result words and the masks; and the
    map's own invariant, count == popcount(mask), on what was got."""
    out = M.problems(want, got)
    if out == ["kind differs"]:
        return out
    if "result" in want and tuple(want["result"]) != tuple(got.get("result", ())):
        out.append("the eleven result words: expected %s, got %s" % (dict(zip(RESULT_FIELDS, want["result"])), got.get("result")))
    for name in ("counted", "voted"):
        w = want.get(name)
        if w is None:
            continue
        g = got.get(name)
        if g is None or len(g) != len(w):
            out.append("%s is missing or of another length" % name)
        elif not np.array_equal(np.asarray(w, np.uint32), np.asarray(g, np.uint32)):
            k = int(np.flatnonzero(np.asarray(w, np.uint32) != np.asarray(g, np.uint32))[0])
            out.append("%s differs at %d: expected %d, got %d" % (name, k, w[k], g[k]))
    wm, gm = want["state"][3], np.asarray(got["state"][3])
    if wm.shape != gm.shape:
        out.append("state masks: shape %s expected, got %s" % (wm.shape, gm.shape))
    elif not np.array_equal(wm, gm):
        out.append("state masks differs")
    gc = np.asarray(got["state"][2])
    if gm.ndim == 2 and gm.shape[0] == gc.shape[0] and not np.array_equal(popcount(gm), gc):
        out.append("state count is not popcount(mask)")
    return out


# ---------------------------------------------------------------------------------------
# the sequences

sizes = M.sizes


def patterns(n):
    """name -> (rows, voters). distinct: every (key, voter) pair once, four voters a key;
    equal: one key, one voter; random: draws from n / 4 keys x 4 voters."""
    i = np.arange(n, dtype=np.uint32)
    rng = np.random.default_rng(0x707E + n)
    return {"distinct": (i // 4 + 1000, i % 4),
            "equal": (np.full(n, 77, np.uint32), np.full(n, 2, np.uint32)),
            "random": (rng.integers(0, max(1, n // 4), n).astype(np.uint32), rng.integers(0, 4, n).astype(np.uint32))}


def one_call_sequences():
    """One vote on an empty map that fits exactly, then a find_votes of the same slots."""
    out = []
    for n in sizes():
        for name, (val, voter) in patterns(n).items():
            keys = int(np.unique(val).size)
            out.append(VSequence("one_%d_%s" % (n, name), keys, [vote(val, voter, threshold=2), find_votes(val, voter)]))
    return out


BIG = M.BIG                     # 257 tiles: k_vote_scan takes a second chunk of 256


def big_sequence():
    return VSequence("big_exact_fit", BIG, [vote(np.arange(BIG, dtype=np.uint32), 3, threshold=1, crossed_cap=4)], big=True)


EDGE_VOTERS = (0, 31, 32, 63, 64)
MASK_EDGES = (1, 31, 32, 33, 64, 65, 1024)


def mask_edge_sequences():
    """max_voters at the word edges; voters 0, 31, 32, 63, 64 and max_voters - 1 (those at or
    past max_voters are bad voters) on one key, then spread over three keys, then all of
    them again on every key, reversed: repeats where they were counted."""
    out = []
    for mv in MASK_EDGES:
        v = np.array(EDGE_VOTERS + (mv - 1,), dtype=np.uint32)
        spread = np.arange(v.size, dtype=np.uint32) % 3 + 1
        every = np.repeat(np.arange(4, dtype=np.uint32), v.size)
        out.append(VSequence("mask_edges_%d" % mv, 4, [
            vote(np.zeros(v.size, np.uint32), v, threshold=2),
            vote(spread, v, threshold=2),
            vote(every, np.tile(v[::-1], 4), threshold=3, crossed_cap=4),
            find_votes(every, np.tile(v, 4))], max_voters=mv))
    return out


DUP_KEY, DUP_VOTER = 7, 2
DUPLICATES = {"wave": (5, 40), "waves": (5, 200), "tiles": (5, 300), "leader_third": (300, 560)}


def duplicate_sequences():
    """600 slots, every filler slot a key of its own voted for by voter 0, and one equal
    (key, voter) pair at two slots: inside one wave, in two waves of a tile, in two tiles,
    and in tiles 1 and 2 with the key's leader (another voter's slot) in tile 0. Then the
    same slots in reversed order."""
    out = []
    for name, (a, b) in DUPLICATES.items():
        val = np.arange(600, dtype=np.uint32) + 100
        voter = np.zeros(600, np.uint32)
        val[[a, b]] = DUP_KEY
        voter[[a, b]] = DUP_VOTER
        if name == "leader_third":
            val[5], voter[5] = DUP_KEY, 1
        out.append(VSequence("dup_" + name, 600, [vote(val, voter, threshold=2)]))
        out.append(VSequence("dup_" + name + "_reversed", 600, [vote(val[::-1].copy(), voter[::-1].copy(), threshold=2)]))
    return out


def across_sequences():
    A, B, C = 11, 12, 13
    five = np.repeat(np.arange(5, dtype=np.uint32) + 20, 3)
    return [
        VSequence("repeat_later", 8, [vote([A, A, B], [0, 1, 0]), vote([A, B, A], [0, 1, 1]), vote([B, A], [1, 2])]),
        # the slots of M "third_voter_plain": A's count is its slots there, its voters here
        VSequence("third_voter", 8, [vote([A, A, B], [0, 0, 1], threshold=3),
                                     vote([A, A, B], [1, 0, 1], threshold=3),
                                     vote([A], [2], threshold=3)]),
        VSequence("crossing", 16, [vote([A, B, A, C, C, A, A], [0, 0, 1, 0, 1, 1, 2], threshold=2),       # A 0->3, C 0->2
                                   vote([B, B, C], [0, 1, 2], threshold=2),                             # B 1->2
                                   vote([A, B, C], [3, 2, 3], threshold=0),                             # no threshold
                                   vote([B, B], [3, 3], threshold=4, crossed_cap=0),                    # a NULL list
                                   vote([A], [3], threshold=4, crossed_cap=0)], max_voters=8),
        VSequence("crossing_cap", 16, [vote(five, np.tile([0, 1, 1], 5), threshold=2, crossed_cap=2),
                                       vote(five, np.tile([2, 0, 3], 5), threshold=4, crossed_cap=5)]),
    ]


def third_voter_plain():
    """The slots of "third_voter" on a plain map with add: A crosses one call earlier."""
    A, B = 11, 12
    return M.Sequence("third_voter_plain", 8, [M.add([A, A, B], threshold=3), M.add([A, A, B], threshold=3),
                                               M.add([A], threshold=3)])


def bad_voter_sequences():
    out = []
    for mv in (5, 33):
        out.append(VSequence("bad_voters_%d" % mv, 8, [
            vote([1, 2], [mv, ALL32], threshold=1),                                  # alone on new keys: entered, count 0
            vote([1, 3, 3, 2, 3], [mv - 1, mv, 0, ALL32, mv + 1], threshold=1),      # beside good votes
            find_votes([1, 2, 3, 3], [mv - 1, mv, 0, ALL32])], max_voters=mv))
    return out


def full_sequence():
    return VSequence("full", 4, [
        vote([1, 2, 3, 1], [0, 0, 0, 1], threshold=2),
        vote([8, 2, 9, 2, 1], [0, 1, 0, 0, 1], threshold=1),     # two new and two held: refused whole
        find_votes([1, 2, 3, 8, 9, 2], [1, 1, 0, 0, 0, 0]),
        vote([8, 2], [3, 1], threshold=2),                       # one new: id 3; fits exactly
        vote([9], [0]),                                          # one more: refused
        vote([2, 2, 8], [2, 2, 3]),                              # held keys alone still go in
        find_votes([9, 8], [0, 3])])


PAIR_N = 70


def probe_sequences():
    """The pair table's chain: 70 votes on 7 keys x 5 voters, so every pair twice, every
    pair's home forced to 0 and to capacity - 1 (the chain wraps around). The map's chain:
    max_keys 8, capacity 64, every key's home 0 and 63."""
    i = np.arange(PAIR_N, dtype=np.uint32)
    pairs = [vote(i % 7, i // 7 % 5, threshold=3), vote((i * 3) % 7, (i + 2) % 5, threshold=5, crossed_cap=3)]
    out = [VSequence("pair_chain_%d" % h, 8, pairs, max_voters=5, pair_home=h) for h in (0, capacity(PAIR_N) - 1)]
    steps = [vote([1, 2, 3, 2], [0, 0, 0, 1]), find_votes([3, 2, 1, 4], [0, 1, 1, 0]),
             vote([9, 2, 8, 9], [1, 1, 2, 1]), find_votes([8, 9, 1, 2, 3, 7], [2, 0, 0, 1, 3, 0]),
             vote([5, 6, 1, 7, 5], [0, 1, 3, 3, 2]), find_votes(np.arange(12), 3)]
    return out + [VSequence("map_chain_home_%d" % h, 8, steps, home=h) for h in (0, 63)]


def other_sequences():
    a = np.arange(70, dtype=np.uint32) % 9
    v = np.arange(70, dtype=np.uint32) % 3
    return [
        VSequence("no_counts", 16, [vote(a, v, threshold=2, counts=False), vote(a, (v + 1) % 4, threshold=4, counts=False),
                                    find_votes(a, v, counts=False)]),
        VSequence("clear_reuse", 16, [vote(a, v), clear(), find_votes(a, v), vote([4, 100, 3, 4], [1, 1, 0, 1], threshold=1),
                                      clear(), clear(), vote([7], [1])]),
        VSequence("find_votes", 16, [find_votes([1, 2], [0, 1]), vote([1, 2, 1], [0, 3, 2]),
                                     # held and set, held and not set, absent, out of range, set again
                                     find_votes([1, 1, 5, 2, 2], [2, 1, 0, 4, 3]),
                                     find_votes([1, 6], [0, 0], counts=False)]),
        VSequence("scoped", 16, [vote(np.full(12, 9, np.uint32), np.arange(12) % 2, scope=np.arange(12) % 3, threshold=2),
                                 find_votes(np.full(3, 9, np.uint32), [1, 0, 1], scope=[0, 5, 2])]),
    ]


def all_sequences():
    return (one_call_sequences() + [big_sequence()] + mask_edge_sequences() + duplicate_sequences() + across_sequences() +
            bad_voter_sequences() + [full_sequence()] + probe_sequences() + other_sequences())


# ---------------------------------------------------------------------------------------
# the stand-alone check's files

def write_sequences(path, seqs):
    """A count; per sequence five 8-byte words (max_keys, max_voters, forced home of the
    map's table and of the pair table as signed words, steps); per step seven words (kind,
    n, has_scope, threshold, crossed_cap, flips, counts), then, unless a clear, the rows,
    the scopes when there are any, the voters and the flips, each padded to 8 bytes."""
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(seqs)))
        for s in seqs:
            f.write(struct.pack("<5q", s.max_keys, s.max_voters, -1 if s.home is None else s.home,
                                -1 if s.pair_home is None else s.pair_home, len(s.steps)))
            for st in s.steps:
                f.write(struct.pack("<7q", st.kind, st.n, int(st.scope is not None), st.threshold, st.crossed_cap,
                                    len(st.flips), int(st.counts)))
                if st.kind == CLEAR:
                    continue
                f.write(M._words(np.asarray(st.val, dtype="<u4")))
                if st.scope is not None:
                    f.write(M._words(np.asarray(st.scope, dtype="<u4")))
                f.write(M._words(np.asarray(st.voter, dtype="<u4")))
                f.write(M._words(np.asarray(st.flips, dtype="<u4").reshape(-1)))


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
            if st.kind == VOTE:
                r["result"] = tuple(int(x) for x in take("<u8", 11))
                r["ids"] = take("<u4", st.n)
                counted, before, after = take("<u4", st.n), take("<u4", st.n), take("<u4", st.n)
                r["counted"], r["before"], r["after"] = (counted, before, after) if st.counts else (None, None, None)
                r["crossed"] = take("<u4", st.crossed_cap)
            elif st.kind == FIND_VOTES:
                r["ids"] = take("<u4", st.n)
                count = take("<u4", st.n)
                r["count"] = count if st.counts else None
                r["voted"] = take("<u4", st.n)
            entries = int(take("<u8", 1)[0])
            r["state"] = (take("<u4", entries), take("u1", 32 * entries).reshape(-1, 32), take("<u4", entries),
                          take("<u4", entries * words(s.max_voters)).reshape(entries, words(s.max_voters)))
            steps.append(r)
        out.append(steps)
    assert at == len(data)
    return out
