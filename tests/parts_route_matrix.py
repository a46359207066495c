"""The matrix of msha_hash_actions_device_routed (mirbft_amd/csrc/parts_plan.hip
k_route_measure, parts_route.hpp): a reference model of the ROUTE -- which lists are
long, how many of them are routed, which stay lanes -- written from include/mirsha.h,
"Part lists with their long lists routed to the chains", and the case builders of
tests/test_gpu_parts_routed.py. No GPU and no torch: tests/test_parts_route_cpu.py
proves by set equality what the builders reach and that check_route() rejects wrong
routes.

From the header:

  WHAT IS ROUTED  "A list is LONG when some action names it, its part range is valid and
                  msha_blocks_for_len(the sum of its part lengths) >= long_blocks."
  CAPS            "At most max_long lists are routed, and a list is given room only while
                  off + round16(len) + MSHA_DEVICE_ARENA_SLACK <= long_bytes holds for
                  it [...] When every long list fits both caps, exactly the long lists
                  are routed. [...] of long lists of one length L exactly min(n_long,
                  max_long, floor((long_bytes - MSHA_DEVICE_ARENA_SLACK) / round16(L)))
                  are."
  ORDER           "the lanes that remain are in descending block-count class"

Digests are hashlib's of the joined parts, zeros where the header says zeros.
"""
from __future__ import annotations

import hashlib
from collections import namedtuple

import numpy as np

SLACK = 64                      # MSHA_DEVICE_ARENA_SLACK
EXACT = 4096                    # classes: the exact block count below 4,096 blocks
CUS = 256                       # MI355X compute units: the default max_long is 16 x CUS
DEFAULT_LONG_BLOCKS = 64
DEFAULT_LONG_BYTES = 32 << 20
FAR = 1 << 40                   # an offset no arena of these tests reaches

# lists: per list the byte strings hashlib gets, or None for a list that must not be read
Case = namedtuple("Case", "arena part_off part_len begin action_list lists long_blocks max_long long_bytes")
Model = namedtuple("Model", "n_lists named valid long nbytes blocks cls max_long long_bytes all_fit count")


def blocks_for_bytes(nbytes: int) -> int:
    return nbytes // 64 + (1 if nbytes % 64 < 56 else 2)


def round16(x: int) -> int:
    return (x + 15) // 16 * 16


def block_class(blocks: int) -> int:
    return blocks if blocks < EXACT else 1 << (blocks.bit_length() - 1)


# ---- the reference model ----------------------------------------------------------

def route_model(part_len, begin, action_list=None, long_blocks=0, max_long=0, long_bytes=0) -> Model:
    """What the header promises of one call. named: the lists some action names;
    valid: those of them whose part range neither decreases nor spans 2^32 parts; long:
    the valid ones of >= long_blocks blocks. all_fit: every long list finds a slot and
    room, in whatever order they come. count: how many lists are routed -- len(long)
    when all fit, the header's formula when the long lists have one length, else None
    (unspecified)."""
    part_len = [int(x) for x in np.asarray(part_len, dtype=np.uint64).tolist()]
    begin = [int(x) for x in np.asarray(begin, dtype=np.uint64).tolist()]
    n_lists = len(begin) - 1
    long_blocks = long_blocks or DEFAULT_LONG_BLOCKS
    max_long = max_long or 16 * CUS
    long_bytes = long_bytes or DEFAULT_LONG_BYTES
    if action_list is None:
        named = set(range(n_lists))
    else:
        named = {int(x) for x in np.asarray(action_list).tolist() if 0 <= int(x) < n_lists}
    cs = [0]
    for v in part_len:
        cs.append(cs[-1] + v)
    valid, nbytes, blocks, cls = set(), {}, {}, {}
    for l in sorted(named):                       # an unnamed list's range is not even looked at
        b, e = begin[l], begin[l + 1]
        if e < b or e - b > 0xFFFFFFFF:
            nbytes[l], blocks[l], cls[l] = 0, 0, 0   # a lane of no blocks: it sorts last
            continue
        valid.add(l)
        nbytes[l] = cs[e] - cs[b]
        blocks[l] = blocks_for_bytes(nbytes[l])
        cls[l] = block_class(blocks[l])
    long = {l for l in valid if blocks[l] >= long_blocks}
    need = sum(round16(nbytes[l]) for l in long)
    all_fit = len(long) <= max_long and need + SLACK <= long_bytes
    count = None
    if all_fit:
        count = len(long)
    elif len({nbytes[l] for l in long}) == 1:
        L = nbytes[next(iter(long))]
        room = max(long_bytes - SLACK, 0)
        count = min(len(long), max_long, room // round16(L) if L else len(long))
    return Model(n_lists, named, valid, long, nbytes, blocks, cls, max_long, long_bytes, all_fit, count)


def check_route(routed_ids, routed_bytes, order, model: Model) -> list:
    """The problems of a route, [] when it is one the header allows: the routed lists
    are distinct long lists, at most max_long, their rounded lengths sum to routed_bytes
    and fit long_bytes with the slack; every named list is routed or a lane, never both,
    never neither; no unnamed list is either; the routed count is the model's where the
    header fixes it; and the classes never increase along the lane order."""
    routed = [int(x) for x in np.asarray(routed_ids).tolist()]
    order = [int(x) for x in np.asarray(order).tolist()]
    out = []
    if len(set(routed)) != len(routed):
        out.append("a list is routed twice")
    if len(set(order)) != len(order):
        out.append("a list is a lane twice")
    rs, ls = set(routed), set(order)
    for l in sorted(rs - model.named):
        out.append("list %d is routed and no action names it" % l)
    for l in sorted((rs & model.named) - model.long):
        out.append("list %d is routed and is not long (%d blocks)" % (l, model.blocks.get(l, 0)))
    for l in sorted(ls - model.named):
        out.append("list %d is a lane and no action names it" % l)
    for l in sorted(rs & ls):
        out.append("list %d is routed and a lane" % l)
    for l in sorted(model.named - rs - ls):
        out.append("list %d is neither routed nor a lane" % l)
    if len(routed) > model.max_long:
        out.append("%d lists routed, max_long is %d" % (len(routed), model.max_long))
    if rs <= model.long:
        want = sum(round16(model.nbytes[l]) for l in rs)
        if int(routed_bytes) != want:
            out.append("routed_bytes %d, the routed lists' rounded lengths sum to %d" % (routed_bytes, want))
    if int(routed_bytes) + SLACK > model.long_bytes and routed:
        out.append("routed_bytes %d + slack is over long_bytes %d" % (routed_bytes, model.long_bytes))
    if model.count is not None and len(routed) != model.count:
        out.append("%d lists routed, the header says %d" % (len(routed), model.count))
    if model.all_fit and rs != model.long:
        out.append("every long list fits and the routed set is not the long set")
    if ls <= model.named:
        for p in range(1, len(order)):
            if model.cls[order[p]] > model.cls[order[p - 1]]:
                out.append("class increases at lane %d" % p)
                break
    return out


def expected_digests(case: Case) -> np.ndarray:
    """[n_actions, 32]: hashlib of each named list's parts joined; zeros for an action
    whose id is out of range or whose list's part range is invalid."""
    n_lists = case.begin.size - 1
    m = route_model(case.part_len, case.begin, case.action_list, case.long_blocks, case.max_long, case.long_bytes)
    per = {}
    for l in m.named:
        per[l] = hashlib.sha256(b"".join(case.lists[l])).digest() if l in m.valid else bytes(32)
    ids = range(n_lists) if case.action_list is None else [int(x) for x in case.action_list.tolist()]
    rows = [per[i] if 0 <= i < n_lists else bytes(32) for i in ids]
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(-1, 32)


def model_of(case: Case) -> Model:
    return route_model(case.part_len, case.begin, case.action_list, case.long_blocks, case.max_long, case.long_bytes)


# ---- building a call ----------------------------------------------------------------

class _Batch:
    """Parts stored back to back behind one odd byte, so starts take every residue."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.buf = bytearray(b"\x5a")
        self.off, self.len, self.begin, self.lists = [], [], [0], []

    def add(self, parts, readable=True) -> int:
        for p in parts:
            if readable:
                self.off.append(len(self.buf))
                self.buf += p
            else:
                self.off.append(FAR + 16 * len(self.off) + 3)
            self.len.append(len(p))
        self.begin.append(len(self.off))
        self.lists.append([bytes(p) for p in parts] if readable else None)
        return len(self.lists) - 1

    def add_bytes(self, nbytes, n_parts=1, readable=True) -> int:
        msg = self.rng.bytes(nbytes)
        cuts = sorted(int(c) for c in self.rng.integers(0, nbytes + 1, size=n_parts - 1))
        edges = [0] + cuts + [nbytes]
        return self.add([msg[a:b] for a, b in zip(edges, edges[1:])], readable)

    def case(self, action_list=None, long_blocks=0, max_long=0, long_bytes=0) -> Case:
        arena = np.frombuffer(bytes(self.buf) + b"\xee" * SLACK, dtype=np.uint8).copy()
        al = None if action_list is None else np.asarray(action_list, dtype=np.uint32)
        return Case(arena, np.array(self.off, dtype=np.uint64), np.array(self.len, dtype=np.uint64),
                    np.array(self.begin, dtype=np.uint64), al, self.lists, long_blocks, max_long, long_bytes)


EDGE_LONG_BLOCKS = 4
EDGE_LENGTHS = tuple(base + past for base in (64, 128, 192) for past in (55, 56, 64))   # 2..5 blocks
EDGE_REPEAT = 300


def threshold_edge(seed: int = 0x7E0) -> Case:
    """long_blocks = 4 and lists of 55, 56 and 64 bytes past 64, 128 and 192: 2, 3, 3, 3,
    4, 4, 4, 5 and 5 blocks, the padding edge of blocks_for_len on the threshold. Three
    copies of the nine: named once, named 300 times, and unnamed -- the unnamed ones'
    parts point far outside the arena. A few one-block lists between them."""
    b = _Batch(seed)
    once, often, never = [], [], []
    for k, n in enumerate(EDGE_LENGTHS):
        once.append(b.add_bytes(n, 1 + k % 3))
        b.add_bytes(7 + k)                                       # short, named once below
        often.append(b.add_bytes(n, 2 + k % 2))
        never.append(b.add_bytes(n, 2, readable=False))
    shorts = [l for l in range(len(b.lists)) if l not in once + often + never]
    al = once + shorts + often * EDGE_REPEAT
    al = b.rng.permutation(np.array(al, dtype=np.uint32))
    return b.case(al, long_blocks=EDGE_LONG_BLOCKS), (once, often, never)


def summing_paths(seed: int = 0x5B3) -> Case:
    """A long list of 3 parts, the middle one 2,000 bytes at an odd offset (the lane sum;
    the copy's cooperative path); a long list of 300 parts of 0..40 bytes, empty ones
    among them (the wave sum at the default threshold; past the copy's 256-part step);
    and short lists around them. Action i is list i."""
    b = _Batch(seed)
    for n in (5, 70, 130):
        b.add_bytes(n)
    b.buf += b"\x00" * ((16 - len(b.buf) % 16) % 16 + 4)         # the 2,000-byte part starts at residue 4 + 5
    three = b.add([b.rng.bytes(5), b.rng.bytes(2000), b.rng.bytes(7)])
    b.add_bytes(40, 2)
    lens = [int(x) for x in b.rng.integers(1, 41, size=300)]
    for k in range(0, 300, 17):
        lens[k] = 0
    many = b.add([b.rng.bytes(n) for n in lens])
    b.add_bytes(64)
    return b.case(None, long_blocks=8), (three, many)


def one_wave_of_long(seed: int = 0x70, n_long: int = 70, parts: int = 33) -> Case:
    """70 consecutive long lists of 33 parts each (every one summed by its wave, one
    after the other: a full wave of them and six more) after three short ones."""
    b = _Batch(seed)
    for n in (3, 60, 100):
        b.add_bytes(n)
    for k in range(n_long):
        b.add_bytes(300 + 16 * (k % 5), parts)
    return b.case(None, long_blocks=5)


CAP_LEN = 1000                                                   # round16: 1,008 bytes, 16 blocks


def caps(max_long=0, long_bytes=0, seed: int = 0xCA9, n_long: int = 5) -> Case:
    """Five long lists of one length among short ones, under the caps given."""
    b = _Batch(seed)
    al = []
    for k in range(n_long):
        al.append(b.add_bytes(20 + k, 2))
        al.append(b.add_bytes(CAP_LEN, 3 + k))
    al.append(b.add_bytes(100))
    return b.case(np.array(al[::-1], dtype=np.uint32), long_blocks=16, max_long=max_long, long_bytes=long_bytes)


def uniform(n_lists: int, long: bool, with_list: bool, seed: int = 0x11F) -> Case:
    """n_lists lists of 90..120 bytes in two parts (two blocks): none long at the
    default threshold, every one long at long_blocks = 2. With an action list every
    list is named, some twice, in reverse."""
    b = _Batch(seed + n_lists)
    for k in range(n_lists):
        b.add_bytes(90 + k % 30, 2)
    al = None
    if with_list:
        al = np.concatenate([np.arange(n_lists)[::-1], np.arange(0, n_lists, 7)]).astype(np.uint32)
    return b.case(al, long_blocks=2 if long else 0)


def empty_long(seed: int = 0xE0) -> Case:
    """long_blocks = 1: every named valid list is long, the empty ones too -- a list of no
    parts, one of a single empty part, one of three empty parts -- between lists of 1, 55,
    56 and 200 bytes. An empty list is given no room (round16(0) = 0): it shares its
    offset with the next claimant and is hashed as the empty message. List 3 is unnamed."""
    b = _Batch(seed)
    b.add_bytes(1)
    b.add([])
    b.add([b""])
    b.add_bytes(77, readable=False)
    b.add_bytes(55, 2)
    b.add([b"", b"", b""])
    b.add_bytes(56)
    b.add_bytes(200, 3)
    return b.case(np.array([7, 1, 2, 0, 5, 4, 6, 1, 5], dtype=np.uint32), long_blocks=1)


def decreasing_long(seed: int = 0xDEC) -> Case:
    """List 2's part range decreases; the parts between its two bounds are 3,000 bytes,
    long by any reading. List 4 is long and valid. The action list names every list and
    one id out of range."""
    b = _Batch(seed)
    b.add_bytes(10)
    b.add_bytes(3000, 4)
    b.add_bytes(50)                                              # list 2, made to decrease below
    b.add_bytes(30)
    b.add_bytes(700, 5)
    c = b.case(np.array([0, 1, 2, 3, 4, 2, 5, 0], dtype=np.uint32), long_blocks=8)
    begin = c.begin.copy()
    begin[2], begin[3] = begin[2], begin[1]                      # list 2 = [begin[2], begin[1]): decreases
    lists = list(c.lists)
    lists[2] = None
    # list 3 now runs from begin[1]: lists 1's and 2's parts and its own
    lists[3] = c.lists[1] + c.lists[2] + c.lists[3]
    return c._replace(begin=begin, lists=lists)


def mixed_batch(seed: int = 0x4096, n_actions: int = 4096) -> Case:
    """One-part lists, 20-part lists and five long ones (80..1,500 blocks), 4,096
    actions naming them at random, every long one at least once."""
    b = _Batch(seed)
    for k in range(600):
        if k % 3 == 0:
            b.add_bytes(int(b.rng.integers(200, 900)), 20)
        else:
            b.add_bytes(int(b.rng.integers(0, 300)))
    longs = []
    for nbytes, parts in ((5100, 40), (96000, 1700), (20000, 3), (8000, 300), (33333, 31)):
        at = b.add_bytes(nbytes, parts)
        longs.append(at)
        b.add_bytes(33)
    al = b.rng.integers(0, len(b.lists), size=n_actions).astype(np.uint32)
    al[[7, 1000, 2000, 3000, 4095]] = longs
    return b.case(al), longs
