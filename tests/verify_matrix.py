"""The cases and the oracle of msha_verify_digests_device (include/mirsha.h "Digests
verified on the GPU"), shared by the CPU check (tests/test_verify_cpu.py, which replays
mirbft_amd/csrc/verify.hpp under sanitizers) and the GPU test (tests/test_gpu_verify.py).

The oracle is numpy written from the header's contract: the mask by np.packbits-style
bit placement, the counts, the first index and the list. It is never the code under
test.

A case is small to describe: row r of the expected table is base_rows(r), slot i holds
the row its index names (an out-of-range index: the row of i itself, which is as good
as anything), and a short list of flips then changes one byte each on either side. The
stand-alone check rebuilds the arrays from that description (write_cases)."""
import os
import re
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "mirbft_amd", "csrc", "verify.hpp")

LIST_SENTINEL = 0xA5A5A5A5      # d_bad_list is prefilled with it: entries at and past `listed` keep it
MASK_PREFILL = 0xFF             # d_bad_mask is prefilled with it: every word has to be rewritten
FLIP = 0x5A                     # a flip xors one byte with it
GOT, EXPECTED = 0, 1            # the side a flip changes
DEFAULT_CAP = 16


def _constant(name):
    text = open(HEADER).read()
    v = re.search(r"constexpr uint32_t %s = (\w+);" % name, text).group(1)
    return int(v) if v.isdigit() else _constant(v)


def scan_words():
    """verify::kScanWords, read from the header (msha_verify_stats.scan_words on the GPU)."""
    return _constant("kScanWords")


def base_rows(r):
    """Row r of the tables: dword k = r * 0x9E3779B1 + k * 0x85EBCA6B mod 2^32, little
    endian. The multiplier is odd, so rows of different r differ (in dword 0 already)."""
    r = np.asarray(r, dtype=np.uint64).reshape(-1, 1)
    k = np.arange(8, dtype=np.uint64).reshape(1, 8)
    w = (r * np.uint64(0x9E3779B1) + k * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    return w.astype("<u4").view(np.uint8).reshape(-1, 32)


@dataclass
class Case:
    name: str
    n: int
    n_expected: int
    list_cap: int = DEFAULT_CAP
    idx: object = None                              # np.uint32[n], or None: slot i expects row i
    flips: list = field(default_factory=list)       # (side, row, byte)

    def arrays(self):
        """-> (got uint8[32 n], expected uint8[32 n_expected])"""
        e = np.arange(self.n, dtype=np.uint64) if self.idx is None else self.idx.astype(np.uint64)
        own = np.arange(self.n, dtype=np.uint64)
        got = base_rows(np.where(e < self.n_expected, e, own)).copy()
        expected = base_rows(np.arange(self.n_expected, dtype=np.uint64)).copy()
        for side, row, byte in self.flips:
            (got if side == GOT else expected)[row, byte] ^= FLIP
        return got.reshape(-1), expected.reshape(-1)


def oracle(got, expected, idx, n_expected, list_cap):
    """The contract restated: -> (mask uint64[ceil(n/64)], (n, bad, first_bad, listed,
    bad_index), list uint32[list_cap] with LIST_SENTINEL at and past listed)."""
    n = got.size // 32
    e = np.arange(n, dtype=np.uint64) if idx is None else np.asarray(idx).astype(np.uint64)
    out_of_range = e >= n_expected
    diff = out_of_range.copy()
    if n_expected:
        rows = expected.reshape(n_expected, 32)[np.where(out_of_range, 0, e).astype(np.int64)]
        diff |= (got.reshape(n, 32) != rows).any(axis=1)
    words = (n + 63) // 64
    bits = np.zeros(64 * words, dtype=np.uint8)
    bits[:n] = diff
    mask = np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)
    slots = np.flatnonzero(diff)
    bad = int(slots.size)
    listed = min(bad, list_cap)
    lst = np.full(list_cap, LIST_SENTINEL, dtype=np.uint32)
    lst[:listed] = slots[:listed]
    return mask, (n, bad, int(slots[0]) if bad else n, listed, int(out_of_range.sum())), lst


def case_oracle(c):
    got, expected = c.arrays()
    return oracle(got, expected, c.idx, c.n_expected, c.list_cap)


def _differ(name, n, slots, list_cap=DEFAULT_CAP):
    """Slots `slots` differ, each in one byte of the got side (byte 7 slot mod 32)."""
    return Case(name, n, n, list_cap, None, [(GOT, int(s), (7 * int(s)) % 32) for s in slots])


def sizes(W):
    """The wave (64), workgroup (256) and scan-chunk (64 W slots) edges."""
    return [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 64 * W - 1, 64 * W, 64 * W + 1, 2 * 64 * W + 1]


def patterns(n, W):
    """name -> differing slots, for a size n; a pattern that needs more slots than n has is left out."""
    rng = np.random.default_rng(0x7E21F ^ n)
    p = {"none": [], "all": range(n), "first": [0], "last": [n - 1]}
    if n > 64:
        p["word_edge"] = [63, 64]                   # the last bit of one word and the first of the next
    if n > 64 * W:
        p["chunk_edge"] = [64 * W - 1, 64 * W]      # one on each side of a scan-chunk edge
    p["random"] = sorted(rng.choice(n, max(1, n // 100), replace=False).tolist())
    return p


def size_cases(n, W):
    return [_differ("n%d_%s" % (n, k), n, v) for k, v in patterns(n, W).items()]


def byte_cases():
    """n = 65, slot 40's EXPECTED digest differs in exactly one byte, position 0 to 31."""
    return [Case("byte%d" % b, 65, 65, DEFAULT_CAP, None, [(EXPECTED, 40, b)]) for b in range(32)]


def list_cases(W):
    """list_cap in {0, 1, bad - 1, bad, bad + 1} at n = 4097; and, at n = 2 * 64 W + 1
    with every 97th slot differing, list_cap in the middle of the second scan chunk and
    exactly on the first chunk's edge (as many as the first chunk holds)."""
    rng = np.random.default_rng(0x115)
    slots = sorted(rng.choice(4097, 40, replace=False).tolist())
    out = [_differ("cap%d" % cap, 4097, slots, cap) for cap in (0, 1, 39, 40, 41)]
    n = 2 * 64 * W + 1
    every = list(range(5, n, 97))
    in_first = sum(1 for s in every if s < 64 * W)
    in_second = sum(1 for s in every if 64 * W <= s < 2 * 64 * W)
    out.append(_differ("cap_mid_chunk", n, every, in_first + in_second // 2))
    out.append(_differ("cap_on_chunk_edge", n, every, in_first))
    return out


def index_cases():
    """Repeats (4 rows shared by 257 slots), a permutation, and indices out of range
    (equal to n_expected, and 0xFFFFFFFF) among valid ones."""
    rng = np.random.default_rng(0x1D8)
    rep = Case("idx_repeats", 257, 4, DEFAULT_CAP, (np.arange(257) % 4).astype(np.uint32),
               [(GOT, 0, 0), (GOT, 100, 31), (GOT, 256, 16)])
    perm = Case("idx_permutation", 4097, 4097, DEFAULT_CAP, rng.permutation(4097).astype(np.uint32),
                [(GOT, 64, 3), (GOT, 4096, 12), (EXPECTED, 9, 20)])
    idx = rng.integers(0, 200, 300).astype(np.uint32)
    idx[5], idx[77], idx[299] = 200, 0xFFFFFFFF, 200
    oob = Case("idx_out_of_range", 300, 200, DEFAULT_CAP, idx, [(GOT, 6, 1), (GOT, 150, 30)])
    return [rep, perm, oob]


def all_cases(W):
    out = []
    for n in sizes(W):
        out += size_cases(n, W)
    return out + byte_cases() + list_cases(W) + index_cases()


def write_cases(path, cases):
    """The description the stand-alone check reads: a count, then per case six 8-byte
    words (n, n_expected, has_idx, list_cap, flips, 0), the indices (4 n bytes, padded to
    8) and the flips as (side, row, byte) 4-byte triples (padded to 8)."""
    with open(path, "wb") as f:
        f.write(np.array([len(cases)], dtype="<u8").tobytes())
        for c in cases:
            has_idx = c.idx is not None
            f.write(np.array([c.n, c.n_expected, int(has_idx), c.list_cap, len(c.flips), 0], dtype="<u8").tobytes())
            for a in ([c.idx.astype("<u4")] if has_idx else []) + [np.array(c.flips, dtype="<u4").reshape(-1)]:
                b = a.tobytes()
                f.write(b + b"\0" * (-len(b) % 8))


def read_results(path, cases):
    """What the check wrote, per case: (mask, result tuple, whole list)."""
    raw = np.fromfile(path, dtype="<u8")
    out, p = [], 0
    for c in cases:
        words = (c.n + 63) // 64
        res = tuple(int(x) for x in raw[p:p + 5])
        mask = raw[p + 5:p + 5 + words].astype(np.uint64)
        p += 5 + words
        lw = (c.list_cap + 1) // 2
        lst = raw[p:p + lw].view("<u4")[:c.list_cap].astype(np.uint32)
        p += lw
        out.append((mask, res, lst))
    assert p == raw.size
    return out


def problems(want, got):
    """Differences between an oracle triple and a result triple, in words."""
    out = []
    (wm, wr, wl), (gm, gr, gl) = want, got
    if tuple(gr) != tuple(wr):
        out.append("result (n, bad, first_bad, listed, bad_index) is %s, expected %s" % (tuple(gr), tuple(wr)))
    if gm.shape != wm.shape or not np.array_equal(gm, wm):
        k = int(np.flatnonzero(gm != wm)[0]) if gm.shape == wm.shape else -1
        out.append("mask differs (first at word %d: %s, expected %s)"
                   % (k, hex(int(gm[k])) if k >= 0 else "?", hex(int(wm[k])) if k >= 0 else "?"))
    if gl.shape != wl.shape or not np.array_equal(gl, wl):
        k = int(np.flatnonzero(gl != wl)[0]) if gl.shape == wl.shape else -1
        out.append("list differs (first at entry %d: %s, expected %s)"
                   % (k, hex(int(gl[k])) if k >= 0 else "?", hex(int(wl[k])) if k >= 0 else "?"))
    return out
