"""The cases and the oracle of msha_group_digests_device (include/mirsha.h "Digests
grouped by value on the GPU"), shared by the CPU check (tests/test_group_cpu.py, which
replays mirbft_amd/csrc/group.hpp under sanitizers) and the GPU test
(tests/test_gpu_group.py).

The oracle is numpy written from the header's contract: np.unique over the 36-byte keys,
the groups renumbered by ascending first index. It is never the code under test.

A case is small to describe: slot i holds row base_rows(val[i]) under scope[i], and a
short list of flips then changes one byte each. The stand-alone check rebuilds the arrays
from that description (write_cases)."""
import os
import re
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "mirbft_amd", "csrc", "group.hpp")

SENTINEL = 0xA5A5A5A5           # every output array is prefilled with it: unwritten entries keep it
FLIP = 0x5A                     # a flip xors one byte with it
DEFAULT_CAP = 16
HOME_NONE, HOME_WRAP = -1, -2   # Case.home: the hash decides; capacity - 2 (the chain wraps around)


def _constant(name):
    text = open(HEADER).read()
    v = re.search(r"constexpr uint32_t %s = (\w+);" % name, text).group(1)
    return int(v, 0) if v[0].isdigit() else _constant(v)


def tile():
    """group::kTile: the slots of one workgroup of the per-slot kernels."""
    return _constant("kTile")


def scan_slots():
    """The slots one chunk of k_group_scan covers: kScanTiles tiles."""
    return _constant("kScanTiles") * tile()


def capacity(n):
    """The header's rule restated: bit_ceil(2 n), at least one wave's worth."""
    c = 64
    while c < 2 * n:
        c *= 2
    return c


def base_rows(r):
    """Row r: dword k = r * 0x9E3779B1 + k * 0x85EBCA6B mod 2^32, little endian. The
    multiplier is odd, so rows of different r differ (in dword 0 already)."""
    r = np.asarray(r, dtype=np.uint64).reshape(-1, 1)
    k = np.arange(8, dtype=np.uint64).reshape(1, 8)
    w = (r * np.uint64(0x9E3779B1) + k * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    return w.astype("<u4").view(np.uint8).reshape(-1, 32)


@dataclass
class Case:
    name: str
    val: object                                     # np.uint32[n]: the row slot i holds
    scope: object = None                            # np.uint32[n], or None: d_scope NULL
    group_cap: int = DEFAULT_CAP
    flips: list = field(default_factory=list)       # (slot, byte)
    home: int = HOME_NONE                           # MSHA_GROUP_FORCE_HOME, or HOME_NONE / HOME_WRAP

    @property
    def n(self):
        return int(self.val.size)

    def force_home(self):
        """The value of MSHA_GROUP_FORCE_HOME, or None."""
        if self.home == HOME_NONE:
            return None
        return capacity(self.n) - 2 if self.home == HOME_WRAP else self.home

    def digests(self):
        """-> uint8[32 n]"""
        d = base_rows(self.val).copy()
        for slot, byte in self.flips:
            d[slot, byte] ^= FLIP
        return d.reshape(-1)


def oracle(digests, scope, group_cap):
    """The contract restated: -> (first, group, members (uint32[n] each), group_first,
    group_count (uint32[group_cap], SENTINEL at and past listed), (n, groups, listed,
    max_count, max_group))."""
    n = digests.size // 32
    keys = np.zeros((n, 36), dtype=np.uint8)
    if scope is not None:
        keys[:, :4] = np.asarray(scope).astype("<u4").view(np.uint8).reshape(n, 4)
    keys[:, 4:] = digests.reshape(n, 32)
    _, index, inverse, counts = np.unique(keys, axis=0, return_index=True, return_inverse=True, return_counts=True)
    inverse = np.asarray(inverse).reshape(-1)
    order = np.argsort(index, kind="stable")        # unique rows by ascending first occurrence
    number = np.empty(order.size, dtype=np.int64)
    number[order] = np.arange(order.size)
    groups = int(order.size)
    listed = min(groups, group_cap)
    group_first = np.full(group_cap, SENTINEL, dtype=np.uint32)
    group_count = np.full(group_cap, SENTINEL, dtype=np.uint32)
    group_first[:listed] = index[order][:listed]
    group_count[:listed] = counts[order][:listed]
    by_number = counts[order]
    max_group = int(np.argmax(by_number))           # the first of the maxima: the smallest id
    return (index[inverse].astype(np.uint32), number[inverse].astype(np.uint32), counts[inverse].astype(np.uint32),
            group_first, group_count, (n, groups, listed, int(by_number[max_group]), max_group))


def case_oracle(c):
    return oracle(c.digests(), c.scope, c.group_cap)


def sizes():
    """The wave (64), tile (T) and scan-chunk (S slots) edges."""
    T, S = tile(), scan_slots()
    return [1, 2, 63, 64, 65, 255, 256, 257, 8 * T - 1, 8 * T + 1, S - 1, S, S + 1, 2 * S + 1]


def patterns(n):
    """name -> the row of every slot, for a size n."""
    i = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(0x6209 ^ n)
    last = np.zeros(n, dtype=np.int64)
    last[n - 1] = 1                                 # its leader is the last slot
    return {"distinct": i, "one": np.zeros(n, dtype=np.int64), "two": i % 2,
            "mirrored": np.minimum(i, n - 1 - i),   # slot i equals slot n - 1 - i: every leader in the first half
            "last_leader": last, "random": rng.integers(0, max(1, n // 10), n)}


def size_cases(n):
    return [Case("n%d_%s" % (n, k), v.astype(np.uint32)) for k, v in patterns(n).items()]


def byte_cases():
    """n = 65, slot 40 holds slot 3's row except for byte b, for every b."""
    val = np.arange(65, dtype=np.uint32)
    val[40] = 3
    return [Case("byte%d" % b, val.copy(), None, DEFAULT_CAP, [(40, b)]) for b in range(32)]


def scope_cases():
    """One digest under three scopes; scopes that differ in bit 31 alone; all-zero scopes
    and, last, the same rows with d_scope NULL."""
    i = np.arange(96, dtype=np.uint32)
    rng = np.random.default_rng(0x5C0)
    rows = rng.integers(0, 9, 96).astype(np.uint32)
    return [Case("scope_three", np.zeros(96, np.uint32), i % 3),
            Case("scope_bit31", np.zeros(96, np.uint32), (i & 1) << 31),
            Case("scope_zero", rows, np.zeros(96, np.uint32)),
            Case("scope_null", rows.copy(), None)]


CAP_GROUPS = 30


def cap_cases():
    """group_cap in {0, 1, groups - 1, groups, groups + 1} over 300 slots of 30 rows."""
    rng = np.random.default_rng(0xCA9)
    val = np.concatenate([rng.permutation(CAP_GROUPS), rng.integers(0, CAP_GROUPS, 300 - CAP_GROUPS)]).astype(np.uint32)
    return [Case("cap%d" % cap, val.copy(), None, cap) for cap in (0, 1, CAP_GROUPS - 1, CAP_GROUPS, CAP_GROUPS + 1)]


def probe_cases():
    """n = 300 with every key's home forced to 0, and to capacity - 2 so that the chain
    wraps around: all distinct (a chain of 300), and a mix of 40 rows with duplicates."""
    rng = np.random.default_rng(0x9B0BE)
    mix = rng.integers(0, 40, 300).astype(np.uint32)
    out = []
    for home, tag in ((0, "home0"), (HOME_WRAP, "wrap")):
        out.append(Case("probe_distinct_" + tag, np.arange(300, dtype=np.uint32), None, DEFAULT_CAP, [], home))
        out.append(Case("probe_mix_" + tag, mix.copy(), None, DEFAULT_CAP, [], home))
    return out


def seed_case():
    rng = np.random.default_rng(0x5EED)
    return Case("seeds", rng.integers(0, 500, 5000).astype(np.uint32), (rng.integers(0, 3, 5000)).astype(np.uint32))


def all_cases():
    out = []
    for n in sizes():
        out += size_cases(n)
    return out + byte_cases() + scope_cases() + cap_cases() + probe_cases() + [seed_case()]


def _padded(a):
    b = a.tobytes()
    return b + b"\0" * (-len(b) % 8)


def write_cases(path, cases):
    """The description the stand-alone check reads: a count, then per case six 8-byte
    words (n, has_scope, group_cap, flips, forced home as a signed word, 0), the rows
    (4 n bytes, padded to 8), the scopes likewise when there are any, and the flips as
    (slot, byte) 4-byte pairs."""
    with open(path, "wb") as f:
        f.write(np.array([len(cases)], dtype="<u8").tobytes())
        for c in cases:
            home = c.force_home()
            f.write(np.array([c.n, int(c.scope is not None), c.group_cap, len(c.flips),
                              -1 if home is None else home, 0], dtype="<i8").tobytes())
            f.write(_padded(c.val.astype("<u4")))
            if c.scope is not None:
                f.write(_padded(c.scope.astype("<u4")))
            f.write(_padded(np.array(c.flips, dtype="<u4").reshape(-1)))


def read_results(path, cases):
    """What the check wrote, per case, in the oracle's shape."""
    raw = np.fromfile(path, dtype="<u8")
    out, p = [], 0

    def take(count):
        nonlocal p
        words = (count + 1) // 2
        a = raw[p:p + words].view("<u4")[:count].astype(np.uint32)
        p += words
        return a

    for c in cases:
        res = tuple(int(x) for x in raw[p:p + 5])
        p += 5
        first, group, members = take(c.n), take(c.n), take(c.n)
        out.append((first, group, members, take(c.group_cap), take(c.group_cap), res))
    assert p == raw.size
    return out


def problems(want, got):
    """Differences between an oracle tuple and a result tuple, in words. got[2] (members)
    may be None: a call without d_members."""
    out = []
    if tuple(got[5]) != tuple(want[5]):
        out.append("result (n, groups, listed, max_count, max_group) is %s, expected %s" % (tuple(got[5]), tuple(want[5])))
    for k, name in enumerate(("first", "group", "members", "group_first", "group_count")):
        w, g = want[k], got[k]
        if g is None:
            continue
        if g.shape != w.shape or not np.array_equal(g, w):
            j = int(np.flatnonzero(g != w)[0]) if g.shape == w.shape else -1
            out.append("%s differs (first at entry %d: %s, expected %s)"
                       % (name, j, hex(int(g[j])) if j >= 0 else "?", hex(int(w[j])) if j >= 0 else "?"))
    return out
