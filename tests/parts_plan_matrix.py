"""The planner matrix of msha_hash_actions_device_planned (mirbft_amd/csrc/parts_plan.hip):
a reference model of the PLAN -- which lists are lanes, how many, in which class order
-- and the case builders that drive every scan wave, the big classes, every path of
the wave histogram and the grid edges of the planner's kernels. No GPU and no torch:
tests/test_parts_plan_matrix_cpu.py proves by set equality which cells the builders
reach, tests/test_gpu_parts_plan_matrix.py runs them.

The model follows include/mirsha.h, "Multi-part actions through part LISTS":

  FOLDING "Every list named at least once is hashed exactly once, however many actions
          name it. A list no action names is not hashed".
  ORDER   "the lanes are the named lists, ordered on the GPU inside the call by
          descending block-count class -- the exact block count below 4,096 blocks,
          powers of two from there up [...] The order inside a class is unspecified."

and msha_blocks_for_len's floor(L/64) + (L%64 < 56 ? 1 : 2). A digest can be right
while the plan is wrong (a list twice in the order, a stale lane from the call before,
a class from a wrong length sum), so the GPU tests check the plan itself: check_plan().

Every builder returns (arena, part_off, part_len, begin, action_list or None, lists):
the arrays of one call, the device contract's slack appended to the arena, and the
lists as the byte strings hashlib gets. Every list of every builder, named or not, has
a valid part range inside the arrays. The long lists take their parts from one shared
64 KiB random region -- parts overlap and repeat -- so a call of 100,000 blocks uploads
little more than its part descriptors.
"""
from __future__ import annotations

import functools
import hashlib
import os
import re
from collections import namedtuple

import numpy as np

import parts_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mirbft_amd", "csrc")
SLACK = 64                      # MSHA_DEVICE_ARENA_SLACK (tests/test_parts_plan_matrix_cpu.py compares)
EXACT = 4096                    # mirsha.h ORDER: "the exact block count below 4,096 blocks"
REGION = 64 * 1024

Case = namedtuple("Case", "arena part_off part_len begin action_list lists")
Model = namedtuple("Model", "named lanes block_sum nbytes blocks cls")


# ---- the reference model ----------------------------------------------------------

def blocks_for_bytes(nbytes: int) -> int:
    return nbytes // 64 + (1 if nbytes % 64 < 56 else 2)


def block_class(blocks: int) -> int:
    """The exact block count below 4,096, else 2**floor(log2(blocks))."""
    blocks = int(blocks)
    return blocks if blocks < EXACT else 1 << (blocks.bit_length() - 1)


def plan_model(part_len, begin, action_list=None) -> Model:
    """The plan the header promises for one call. named: the lists that are lanes,
    ascending (all lists without an action_list, else the distinct in-range ids);
    lanes: how many; block_sum: the blocks compressed for them; nbytes, blocks, cls:
    per list (every list, named or not: the builders' lists are all valid)."""
    part_len = np.asarray(part_len, dtype=np.uint64)
    begin = np.asarray(begin, dtype=np.uint64)
    n_lists = begin.size - 1
    cs = [0]
    for v in part_len.tolist():                  # Python ints: no wrap at any length
        cs.append(cs[-1] + v)
    nbytes = [cs[int(e)] - cs[int(b)] for b, e in zip(begin[:-1].tolist(), begin[1:].tolist())]
    blocks = [blocks_for_bytes(x) for x in nbytes]
    cls = [block_class(b) for b in blocks]
    if action_list is None:
        named = list(range(n_lists))
    else:
        named = sorted({int(x) for x in np.asarray(action_list).tolist() if 0 <= int(x) < n_lists})
    return Model(named, len(named), sum(blocks[l] for l in named), nbytes, blocks, cls)


def check_plan(order, model: Model, lanes=None) -> None:
    """AssertionError, naming the first offending position, unless `order` is a
    permutation of the model's named lists (none missing, repeated or unnamed), the
    class never increases along it, and the lane count (`lanes`: the library's own
    figure where the caller has one, else len(order)) is the model's."""
    order = [int(x) for x in np.asarray(order).tolist()]
    named = set(model.named)
    seen = {}
    for p, l in enumerate(order):
        assert l in named, "position %d holds list %d, which no action names" % (p, l)
        assert l not in seen, "position %d repeats list %d (first at position %d)" % (p, l, seen[l])
        seen[l] = p
    for p, (got, want) in enumerate(zip(sorted(order), model.named)):
        assert got == want, "list %d is missing from the order (sorted position %d holds %d)" % (want, p, got)
    assert len(order) >= len(model.named), \
        "list %d is missing from the order (sorted position %d is past its end)" % (model.named[len(order)], len(order))
    assert sorted(order) == model.named
    lanes = len(order) if lanes is None else int(lanes)
    assert lanes == model.lanes, "lane count %d, the model's is %d" % (lanes, model.lanes)
    for p in range(1, len(order)):
        a, b = model.cls[order[p - 1]], model.cls[order[p]]
        assert b <= a, ("class increases at position %d: list %d (%d blocks, class %d) after list %d (%d blocks, "
                        "class %d)" % (p, order[p], model.blocks[order[p]], b, order[p - 1],
                                       model.blocks[order[p - 1]], a))


def expected_digests(lists, action_list=None) -> np.ndarray:
    """[n_actions, 32]: hashlib.sha256 of each list's parts joined; action i = list
    action_list[i] (None: list i). The only source of expected digests."""
    per = np.frombuffer(b"".join(hashlib.sha256(b"".join(parts)).digest() for parts in lists),
                        dtype=np.uint8).reshape(-1, 32)
    return per if action_list is None else per[np.asarray(action_list, dtype=np.int64)]


# ---- where a block count lands in k_parts_scan --------------------------------------

def _constant(path, pattern) -> int:
    m = re.search(pattern, open(os.path.join(CSRC, path)).read())
    assert m, (path, pattern)
    return int(m.group(1))


@functools.lru_cache(maxsize=None)
def scan_shape():
    """(kKeys, keys a scan thread, keys a scan wave, kBigClasses) read from the sources,
    so the coverage proof follows a retuned scan."""
    exact = _constant("parts_plan.hpp", r"constexpr uint32_t kExactBlocks = (\d+);")
    big = _constant("parts_plan.hpp", r"constexpr uint32_t kBigClasses = (\d+);")
    threads = _constant("parts_plan.hip", r"constexpr uint32_t kScanThreads = (\d+);")
    assert exact == EXACT
    keys = big + exact
    per = (keys + threads - 1) // threads
    return keys, per, 64 * per, big


def scan_key(blocks: int) -> int:
    """63 - floor(log2 b) for b >= 4,096, else kKeys - 1 - b: descending classes, key 0 the longest."""
    keys, _, _, _ = scan_shape()
    blocks = int(blocks)
    return 63 - (blocks.bit_length() - 1) if blocks >= EXACT else keys - 1 - blocks


def scan_thread(blocks: int) -> int:
    return scan_key(blocks) // scan_shape()[1]


def scan_wave(blocks: int) -> int:
    return scan_key(blocks) // scan_shape()[2]


# ---- building a call ----------------------------------------------------------------

class _Batch:
    """The arrays of one call under construction. The arena starts with the shared
    random region; lists given as byte strings go behind it through
    parts_matrix.Arena's residues and filler."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.ar = parts_matrix.Arena(self.rng)
        self.region = self.rng.bytes(REGION)
        self.ar.buf += self.region
        self.begin, self.lists = [0], []
        self.tick = 0

    def _residue(self) -> int:
        self.tick += 1
        return (self.tick * 5) % 16          # 5 is coprime to 16: every start residue, evenly

    def add_parts(self, parts) -> int:
        """A list of these byte strings, each stored at a start residue of its own."""
        for p in parts:
            self.ar.put(bytes(p), self._residue())
        self.begin.append(len(self.ar.off))
        self.lists.append([bytes(p) for p in parts])
        return len(self.lists) - 1

    def add_blocks(self, blocks: int, max_part: int = 4096) -> int:
        """A list of exactly `blocks` SHA-256 blocks, its parts (1..max_part bytes each)
        taken from the shared region at cycling start residues."""
        assert blocks >= 1
        if blocks >= 2 and self.rng.integers(0, 3) == 0:
            nbytes = (blocks - 2) * 64 + int(self.rng.integers(56, 64))      # a length block of its own
        else:
            nbytes = (blocks - 1) * 64 + int(self.rng.integers(0, 56))
        assert blocks_for_bytes(nbytes) == blocks
        parts, left = [], nbytes
        while left:
            n = min(left, int(self.rng.integers(1, max_part + 1)))
            r = self._residue()
            at = 16 * int(self.rng.integers(0, (REGION - n - r) // 16 + 1)) + r
            assert at % 16 == r and at + n <= REGION
            self.ar.off.append(at)
            self.ar.len.append(n)
            parts.append(self.region[at:at + n])
            left -= n
        self.begin.append(len(self.ar.off))
        self.lists.append(parts)
        return len(self.lists) - 1

    def case(self, action_list=None) -> Case:
        arena, off, ln = self.ar.arrays(SLACK)
        al = None if action_list is None else np.asarray(action_list, dtype=np.uint32)
        return Case(arena, off, ln, np.array(self.begin, dtype=np.uint64), al, self.lists)


WAVE_EDGE_BLOCKS = (3828, 3827, 3508, 3507, 3188, 3187, 2868, 2867, 2548, 2547, 2228, 2227,
                    1908, 1907, 1588, 1587, 1268, 1267, 948, 947, 628, 627, 308, 307)
BIG_BLOCKS = (4095, 4096, 4097, 8191, 8192, 16383, 16384)
THREAD_BLOCKS = (102, 101, 100, 99, 98)         # one scan thread's five keys, first to last
N_ONE_BLOCK = 40


def scan_waves_batch(seed: int = 0x5CA9, big=BIG_BLOCKS) -> Case:
    """k_parts_scan and the big classes: a list at the first and the last key of every
    populated scan wave, the big classes and their edges, all five key positions of one
    scan thread, 1 and 2 blocks, a zero-part list, and 40 one-block lists between them,
    in a seeded shuffled index order. -> Case (no action list)."""
    b = _Batch(seed)
    want = list(WAVE_EDGE_BLOCKS) + list(big) + list(THREAD_BLOCKS) + [1, 2, 0] + [1] * N_ONE_BLOCK
    for i in b.rng.permutation(len(want)).tolist():
        if want[i] == 0:
            b.add_parts([])                      # zero parts: the empty string, one block
        else:
            b.add_blocks(want[i])
    return b.case()


def reversed_action_list(case: Case, seed: int = 0x5CAA) -> np.ndarray:
    """scan_waves_batch's second way: the lists named last to first, the 8,192-block
    list 50 times, five one-block lists (not the zero-part one) left unnamed."""
    rng = np.random.default_rng(seed)
    m = plan_model(case.part_len, case.begin)
    ones = [l for l in range(len(case.lists)) if m.blocks[l] == 1 and case.lists[l]]
    unnamed = set(int(x) for x in rng.choice(ones, 5, replace=False))
    al = [l for l in reversed(range(len(case.lists))) if l not in unnamed]
    l8192 = m.blocks.index(8192)
    for at in sorted(int(x) for x in rng.integers(0, len(al), 49)):
        al.insert(at, l8192)
    return np.array(al, dtype=np.uint32)


# hist_add (parts_plan.hip), wave by wave. X is the key three workgroups share.
HIST_PATTERNS = frozenset({"all_one_key", "leader_not_lane_0", "only_lane_63", "empty", "odd_lane_0",
                           "odd_lane_31", "odd_lane_63", "distinct_64", "cut_by_grid"})
HIST_SHARED_BLOCKS = 33                          # X: 64 lanes of workgroup 0, 1 of 2, 37 of 4; none of 1 and 3
HIST_LISTS = 5 * 256 - 27
_HIST_LAYOUT = (
    # workgroup 0
    ("all_one_key", HIST_SHARED_BLOCKS), ("leader_not_lane_0", 7), ("only_lane_63", 12), ("odd_lane_0", (5, 64)),
    # workgroup 1
    ("all_one_key", 20), ("empty", None), ("leader_not_lane_0", 20), ("odd_lane_31", (1, 2)),
    # workgroup 2: the one lane of X is the distinct wave's
    ("distinct_64", None), ("odd_lane_63", (64, 5)), ("all_one_key", 7), ("only_lane_63", 41),
    # workgroup 3
    ("only_lane_63", 12), ("empty", None), ("all_one_key", 1), ("odd_lane_31", (20, 7)),
    # workgroup 4: X's third share is the wave the grid cuts (37 lists, 27 lanes past n_lists)
    ("odd_lane_0", (2, 1)), ("all_one_key", 64), ("leader_not_lane_0", 12), ("cut_by_grid", HIST_SHARED_BLOCKS),
)


def hist_batch(seed: int = 0x4157):
    """hist_add's cases, one pattern a wave, over 5 workgroups x 256 lanes less 27.
    -> (Case, [pattern name per wave]). The action list names the valid lanes in a
    shuffled order, 200 of them twice; the holes are valid lists nobody names."""
    b = _Batch(seed)
    named, patterns = [], []
    for w, (pat, arg) in enumerate(_HIST_LAYOUT):
        patterns.append(pat)
        for lane in range(64):
            l = 64 * w + lane
            if l >= HIST_LISTS:
                break
            hole_blocks = 1 + (l * 7) % 64           # a hole is a list like any other, X among them
            if pat in ("all_one_key", "cut_by_grid"):
                blocks, use = arg, True
            elif pat == "leader_not_lane_0":
                blocks, use = (arg, True) if lane else (hole_blocks, False)
            elif pat == "only_lane_63":
                blocks, use = (arg, True) if lane == 63 else (hole_blocks, False)
            elif pat == "empty":
                blocks, use = hole_blocks, False
            elif pat.startswith("odd_lane_"):
                blocks, use = (arg[1] if lane == int(pat[9:]) else arg[0]), True
            else:                                    # distinct_64: 1..64, none in lane order
                blocks, use = 1 + (lane * 27 + 5) % 64, True
            assert b.add_blocks(blocks, max_part=2048) == l
            if use:
                named.append(l)
    assert len(b.lists) == HIST_LISTS
    rng = np.random.default_rng(seed + 1)
    al = np.array(named, dtype=np.uint32)
    al = np.concatenate([al, rng.choice(al, 200, replace=False)])
    rng.shuffle(al)
    return b.case(al), patterns


LIST_EDGES = (1, 63, 64, 65, 255, 256, 257, 4163, 4164, 4165, 4352, 4353)
ACTION_EDGES = ((3, 1), (3, 255), (3, 256), (3, 257), (3, 70001), (4165, 1), (4165, 70001))


def edge_sizes():
    """-> (n_lists values run without an action list, (n_lists, n_actions) pairs)."""
    return LIST_EDGES, ACTION_EDGES


def tiny_batch(n_lists: int, n_actions=None, seed: int = 0x71E5) -> Case:
    """n_lists lists of 0 to 2 parts and 0 to 70 bytes (one block below 56 bytes, two
    from there), mixed; with n_actions an action list that names every list at least
    once where n_actions allows, in a shuffled order."""
    b = _Batch(seed ^ (n_lists << 8) ^ (n_actions or 0))
    for l in range(n_lists):
        k = l % 3 if l % 7 else 0                    # 0, 1 or 2 parts
        nbytes = int(b.rng.integers(0, 71)) if k else 0
        cut = int(b.rng.integers(0, nbytes + 1))
        msg = b.rng.bytes(nbytes)
        b.add_parts([] if k == 0 else [msg] if k == 1 else [msg[:cut], msg[cut:]])
    if n_actions is None:
        return b.case()
    al = b.rng.integers(0, n_lists, n_actions).astype(np.uint32)
    first = b.rng.permutation(n_lists)[:n_actions]
    al[:first.size] = first
    b.rng.shuffle(al)
    return b.case(al)


def mixed_batch(n_lists: int, seed: int, max_blocks: int = 12, n_actions=None) -> Case:
    """n_lists lists of 1..max_blocks blocks (a zero-part list every 17th), the classes
    mixed in index order; with n_actions an action list naming every list at least once."""
    b = _Batch(seed)
    for l in range(n_lists):
        if l % 17 == 5:
            b.add_parts([])
        else:
            b.add_blocks(1 + (l * 7 + l // max_blocks) % max_blocks, max_part=256)     # every class, neighbours differ
    if n_actions is None:
        return b.case()
    al = b.rng.integers(0, n_lists, n_actions).astype(np.uint32)
    al[:n_lists] = b.rng.permutation(n_lists)
    b.rng.shuffle(al)
    return b.case(al)


WAVE_SUM_PART_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 130)
WAVE_SUM_THRESHOLDS = (1, 64, 100000)
EPOCH_CHANGE_AT, LAST_PART_AT = 77, (33, 134)


def wave_sum_batch(epoch_change, seed: int = 0x5A3E) -> Case:
    """The length sum of k_parts_measure: 200 lists whose part counts cycle through
    WAVE_SUM_PART_COUNTS (both sides of one and of two 64-wide strides), parts of 0 to
    40 bytes and every fifth empty; `epoch_change` (the golden 1,505-part one) as list
    77; and as lists 33 and 134 seventy parts whose bytes cross a padding edge only with
    the last one (55 + 1 bytes: two blocks, not one; 119 + 1: three, not two)."""
    b = _Batch(seed)
    for l in range(200):
        if l == EPOCH_CHANGE_AT:
            b.add_parts(epoch_change)
            continue
        if l in LAST_PART_AT:
            head = 55 if l == LAST_PART_AT[0] else 119
            lens = np.zeros(69, dtype=np.int64)
            for at in b.rng.integers(0, 69, head).tolist():
                lens[at] += 1
            assert lens.sum() == head
            b.add_parts([b.rng.bytes(int(n)) for n in lens] + [b.rng.bytes(1)])
            continue
        k = WAVE_SUM_PART_COUNTS[l % len(WAVE_SUM_PART_COUNTS)]
        b.add_parts([b.rng.bytes(0 if j % 5 == 3 else int(b.rng.integers(0, 41))) for j in range(k)])
    return b.case()
