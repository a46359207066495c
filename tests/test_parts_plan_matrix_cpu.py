"""The planner matrix (tests/parts_plan_matrix.py) checked without a GPU: the model's
block counts and classes agree with the library's host helper, the builders reach, by
set equality, every scan wave, key position, histogram pattern and grid edge they
promise, and check_plan() rejects each kind of wrong plan -- the evidence that the GPU
assertions would fail on a subtly wrong planner, with no wrong kernel built or run."""
import os
import re

import numpy as np
import pytest

import parts_plan_matrix as PM
from mirbft_amd import _lib as L
from mirbft_amd.engine import blocks_for_len


def _one_part_model(nbytes):
    return PM.plan_model(np.array([nbytes], dtype=np.uint64), np.array([0, 1], dtype=np.uint64))


def test_block_counts_equal_the_librarys():
    lens = set(range(201))
    for m in range(64, (1 << 20) + 1, 64):
        lens |= {m - 9, m - 8, m - 1, m, m + 1} if m < 4096 or m & (m - 1) == 0 or m % 4096 == 0 else {m - 8, m}
    lens = sorted(lens)
    assert [PM.blocks_for_bytes(x) for x in lens] == [blocks_for_len(x) for x in lens]
    part_len = np.array(lens, dtype=np.uint64)
    m = PM.plan_model(part_len, np.arange(part_len.size + 1, dtype=np.uint64))     # list i = part i
    assert m.nbytes == lens and m.blocks == [blocks_for_len(x) for x in lens]
    assert _one_part_model(0).blocks == [1] == PM.plan_model(np.zeros(0, dtype=np.uint64), [0, 0]).blocks
    assert PM.SLACK == L.MSHA_DEVICE_ARENA_SLACK


@pytest.mark.parametrize("blocks", [4095, 4096, 8191, 8192, 1 << 20, 1 << 40])
def test_classes_follow_the_librarys_block_count(blocks):
    nbytes = (blocks - 1) * 64 + 17
    lib = blocks_for_len(nbytes)
    assert lib == blocks
    want = lib if lib < 4096 else 1 << (lib.bit_length() - 1)
    m = _one_part_model(nbytes)
    assert (m.blocks, m.cls) == ([lib], [want])
    assert want == {4095: 4095, 4096: 4096, 8191: 4096, 8192: 8192, 1 << 20: 1 << 20, 1 << 40: 1 << 40}[blocks]
    # all of 2^k .. 2^(k+1) - 1 is one class, and the next power of two another
    if blocks >= 4096 and blocks & (blocks - 1) == 0:
        assert PM.block_class(2 * blocks - 1) == blocks and PM.block_class(2 * blocks) == 2 * blocks


def test_scan_shape_is_read_from_the_sources():
    keys, per, wave, big = PM.scan_shape()
    text = open(os.path.join(PM.CSRC, "parts_plan.hpp")).read()
    assert re.search(r"kKeys = kBigClasses \+ kExactBlocks;", text)
    assert (keys, per, wave, big) == (4148, 5, 320, 52)
    assert [PM.scan_key(b) for b in (4095, 4096, 4097, 8191, 8192, 16383, 16384)] == [52, 51, 51, 51, 50, 50, 49]
    assert PM.scan_key(1) == keys - 2 and PM.scan_key(0) == keys - 1
    # keys never increase with the block count: ascending keys are descending classes
    ks = [PM.scan_key(b) for b in range(1, 20000)]
    assert all(a >= b for a, b in zip(ks, ks[1:]))


def test_scan_waves_batch_hits_every_wave_end_and_key_position():
    keys, per, wave, big = PM.scan_shape()
    case = PM.scan_waves_batch()
    assert case.action_list is None
    m = PM.plan_model(case.part_len, case.begin)
    got_keys = {PM.scan_key(b) for b in m.blocks}
    # the keys a valid list of at most 16,384 blocks can have: 49 (2^14) .. kKeys - 2 (one block)
    reachable = set(range(PM.scan_key(16384), keys - 1))
    n_waves = (keys + wave - 1) // wave
    assert n_waves == 13 and {PM.scan_wave(b) for b in m.blocks} == set(range(n_waves))
    ends = {k for w in range(n_waves) for k in (wave * w, wave * w + wave - 1)} & reachable
    assert ends == {PM.scan_key(b) for b in PM.WAVE_EDGE_BLOCKS} and len(ends) == 24
    assert ends <= got_keys
    assert {49, 50, 51, 52} <= got_keys and not any(k < 49 for k in got_keys)
    assert {PM.scan_key(b) % per for b in m.blocks} == set(range(per))
    # one scan thread holds a list at each of its keys, the first and the last among them
    assert len({PM.scan_thread(b) for b in PM.THREAD_BLOCKS}) == 1
    assert [PM.scan_key(b) % per for b in PM.THREAD_BLOCKS] == list(range(per))
    assert set(PM.THREAD_BLOCKS) <= set(m.blocks)
    for b in PM.BIG_BLOCKS + (1, 2):
        assert m.blocks.count(b) == (1 if b > 1 else PM.N_ONE_BLOCK + 2), b      # 40, the 1-block list, zero parts
    zero = [l for l, parts in enumerate(case.lists) if not parts]
    assert len(zero) == 1 and m.blocks[zero[0]] == 1 and m.nbytes[zero[0]] == 0
    assert max(m.blocks) == 16384 and 105000 <= m.block_sum <= 120000
    # shuffled: the long lists are not in index order, one-block lists lie between them
    long_at = [l for l in range(len(case.lists)) if m.blocks[l] > 2]
    assert [m.blocks[l] for l in long_at] != sorted((m.blocks[l] for l in long_at), reverse=True)
    assert any(m.blocks[l] == 1 for l in range(long_at[0], long_at[-1]))
    _check_case(case, region_parts=True)
    # the second way: reversed, the 8,192-block list 50 times, five one-block lists unnamed
    al = PM.reversed_action_list(case)
    m2 = PM.plan_model(case.part_len, case.begin, al)
    gone = sorted(set(m.named) - set(m2.named))
    assert len(gone) == 5 and all(m.blocks[l] == 1 and case.lists[l] for l in gone)
    assert int((al == m.blocks.index(8192)).sum()) == 50
    first = [int(x) for x in al.tolist() if x != m.blocks.index(8192)]
    assert first == sorted(first, reverse=True)
    assert m2.lanes == m.lanes - 5 and m2.block_sum == m.block_sum - 5


def _check_case(case, region_parts=False):
    """The arrays are what the contract asks: ranges inside the arrays, every part
    inside the arena with the slack behind it, the byte strings what the arrays say."""
    n_parts = case.part_off.size
    assert case.part_len.size == n_parts and case.begin[0] == 0 and case.begin[-1] == n_parts
    assert (np.diff(case.begin.astype(np.int64)) >= 0).all()
    assert case.begin.size - 1 == len(case.lists)
    end = (case.part_off + case.part_len).max() if n_parts else 0
    assert int(end) + PM.SLACK <= case.arena.size
    raw = case.arena.tobytes()
    for l in (0, len(case.lists) // 2, len(case.lists) - 1):
        parts = [raw[int(case.part_off[j]):int(case.part_off[j] + case.part_len[j])]
                 for j in range(int(case.begin[l]), int(case.begin[l + 1]))]
        assert parts == case.lists[l]
    if region_parts:
        ln = case.part_len[case.part_off < PM.REGION]
        assert ln.min() >= 1 and ln.max() <= 4096 and ln.max() > 4000
        assert {int(o) % 16 for o in case.part_off[case.part_off < PM.REGION]} == set(range(16))
        assert case.arena.size < 2 * PM.REGION          # the upload stays small while the lists are long


def _wave_patterns(blocks, named, n_lists):
    """Each wave's hist_add case, from the arrays alone."""
    out = []
    for w in range((n_lists + 63) // 64):
        lanes = range(64 * w, 64 * w + 64)
        valid = [l < n_lists and l in named for l in lanes]
        ks = [PM.scan_key(blocks[l]) if v else None for l, v in zip(lanes, valid)]
        seen = [k for k in ks if k is not None]
        if 64 * w + 64 > n_lists:
            out.append("cut_by_grid")
        elif not seen:
            out.append("empty")
        elif len(set(seen)) == 1:
            out.append("all_one_key" if len(seen) == 64 else
                       "only_lane_63" if valid == [False] * 63 + [True] else
                       "leader_not_lane_0" if not valid[0] and len(seen) > 1 else "other")
        elif len(set(seen)) == 64:
            out.append("distinct_64")
        elif len(seen) == 64 and len(set(seen)) == 2 and min(seen.count(k) for k in set(seen)) == 1:
            out.append("odd_lane_%d" % next(i for i, k in enumerate(ks) if seen.count(k) == 1))
        else:
            out.append("other")
    return out


def test_hist_batch_hits_exactly_the_named_patterns():
    case, labels = PM.hist_batch()
    n_lists = case.begin.size - 1
    assert n_lists == PM.HIST_LISTS == 5 * 256 - 27
    m = PM.plan_model(case.part_len, case.begin, case.action_list)
    assert set(m.blocks) == set(range(1, 65))
    named = set(m.named)
    got = _wave_patterns(m.blocks, named, n_lists)
    assert got == labels
    assert set(got) == PM.HIST_PATTERNS
    # an empty wave has named waves before and after it in its workgroup
    for w, p in enumerate(got):
        if p == "empty":
            assert w % 4 not in (0, 3) and got[w - 1] != "empty" and got[w + 1] != "empty"
    # the cut wave: 37 lists, all named, one key; 27 lanes past n_lists
    assert got[-1] == "cut_by_grid" and got.count("cut_by_grid") == 1
    tail = range(64 * (len(got) - 1), n_lists)
    assert len(tail) == 37 and all(l in named for l in tail)
    # one bucket shared by workgroups 0, 2 and 4 with 64, 1 and 37 lanes, absent from 1 and 3
    share = [sum(1 for l in range(256 * g, min(256 * g + 256, n_lists))
                 if l in named and m.blocks[l] == PM.HIST_SHARED_BLOCKS) for g in range(5)]
    assert share == [64, 0, 1, 0, 37]
    # holes are real lists, the shared key among them, and some lists are named twice
    holes = [l for l in range(n_lists) if l not in named]
    assert holes and PM.HIST_SHARED_BLOCKS in {m.blocks[l] for l in holes}
    assert case.action_list.size == len(named) + 200 and m.lanes == len(named)
    assert case.action_list.tolist() != sorted(case.action_list.tolist())
    _check_case(case)


def test_edge_sizes_are_the_grid_edges():
    lists, pairs = PM.edge_sizes()
    keys = PM.scan_shape()[0]
    assert set(lists) == {1, 63, 64, 65, 255, 256, 257, 4163, 4164, 4165, 4352, 4353}
    assert set(pairs) == {(3, 1), (3, 255), (3, 256), (3, 257), (3, 70001), (4165, 1), (4165, 70001)}
    assert 16 + keys == 4164 and 4352 % 256 == 0 and 4352 > 4164
    hip = open(os.path.join(PM.CSRC, "parts_plan.hip")).read()
    assert "a.n_lists > 16 + kKeys ? a.n_lists : 16 + kKeys" in hip       # where k_parts_init's grid switches


@pytest.mark.parametrize("n_lists,n_actions", [(257, None), (4165, None), (3, 1), (3, 257), (4165, 1), (4165, 70001)])
def test_tiny_batches_are_tiny_and_name_what_they_can(n_lists, n_actions):
    case = PM.tiny_batch(n_lists, n_actions)
    m = PM.plan_model(case.part_len, case.begin, case.action_list)
    assert len(case.lists) == n_lists
    assert {len(p) for p in case.lists} <= {0, 1, 2} and max(m.nbytes) <= 70
    assert set(m.blocks) <= {1, 2}
    if n_lists > 60:
        assert {len(p) for p in case.lists} == {0, 1, 2} and set(m.blocks) == {1, 2}
    if n_actions is None:
        assert case.action_list is None and m.lanes == n_lists
    else:
        assert case.action_list.size == n_actions and m.lanes == min(n_lists, n_actions)
    _check_case(case)


def test_mixed_batches_mix_their_classes():
    """The sequence test's calls: every class 1..max_blocks, zero-part lists among
    them, neighbours of different classes, every list named where there is an action list."""
    for n_lists, max_blocks, n_actions in ((4501, 12, None), (70, 12, 100000), (300, 40, None)):
        case = PM.mixed_batch(n_lists, seed=0x5E00 + n_lists, max_blocks=max_blocks, n_actions=n_actions)
        m = PM.plan_model(case.part_len, case.begin, case.action_list)
        assert m.lanes == n_lists and set(m.blocks) == set(range(1, max_blocks + 1))
        assert sum(1 for p in case.lists if not p) >= n_lists // 17
        assert sum(1 for a, b in zip(m.blocks, m.blocks[1:]) if a != b) > n_lists // 2
        assert case.action_list is None or case.action_list.size == n_actions
        _check_case(case)


def test_wave_sum_batch_shape():
    ec = [bytes([j & 255]) * (1 + j % 9) for j in range(1505)]
    case = PM.wave_sum_batch(ec)
    counts = np.diff(case.begin.astype(np.int64)).tolist()
    assert len(counts) == 200 and counts[PM.EPOCH_CHANGE_AT] == 1505
    for l, c in enumerate(counts):
        if l != PM.EPOCH_CHANGE_AT and l not in PM.LAST_PART_AT:
            assert c == PM.WAVE_SUM_PART_COUNTS[l % 10]
    assert sum(1 for c in counts[:64] if c) >= 50           # the pending loop's turns in wave 0 at T = 1
    rest = [n for l in range(200) if l != PM.EPOCH_CHANGE_AT for n in map(len, case.lists[l])]
    assert min(rest) == 0 and max(rest) == 40 and rest.count(0) > 100
    m = PM.plan_model(case.part_len, case.begin)
    for l, (head, blocks) in zip(PM.LAST_PART_AT, ((55, 2), (119, 3))):
        assert counts[l] == 70 and sum(map(len, case.lists[l][:-1])) == head and len(case.lists[l][-1]) == 1
        assert PM.blocks_for_bytes(head) == blocks - 1 and m.blocks[l] == blocks
    assert set(PM.WAVE_SUM_THRESHOLDS) == {1, 64, 100000}
    _check_case(case)


def _good_plan():
    """A correct plan over six classes, 4,096 and 8,191 blocks among them, list 3 unnamed."""
    blocks = [2, 8191, 1, 7, 4096, 16384, 2, 1, 4095]
    part_len = np.array([(b - 1) * 64 for b in blocks], dtype=np.uint64)
    al = np.array([8, 0, 1, 2, 4, 5, 6, 7, 7, 0], dtype=np.uint32)
    m = PM.plan_model(part_len, np.arange(len(blocks) + 1, dtype=np.uint64), al)
    assert m.named == [0, 1, 2, 4, 5, 6, 7, 8] and m.lanes == 8 and m.blocks == blocks
    return [5, 1, 4, 8, 0, 6, 2, 7], m


def test_check_plan_rejects_every_kind_of_wrong_plan():
    order, m = _good_plan()
    PM.check_plan(order, m)
    PM.check_plan(np.array(order, dtype=np.uint32), m, lanes=8)
    PM.check_plan([5, 4, 1, 8, 6, 0, 7, 2], m)              # 4,096 and 8,191 blocks either way round; so equal counts
    wrong = {
        "dropped": (order[:3] + order[4:], None, r"list 8 is missing"),
        "repeated": ([5, 1, 4, 8, 0, 0, 2, 7], None, r"position 5 repeats list 0 \(first at position 4\)"),
        "unnamed": ([5, 1, 4, 8, 3, 0, 6, 2, 7], None, r"position 4 holds list 3, which no action names"),
        "swapped": ([5, 1, 4, 0, 8, 6, 2, 7], None, r"class increases at position 4: list 8 \(4095 blocks"),
        "lane count": (order, 9, r"lane count 9, the model's is 8"),
    }
    messages = {}
    for name, (plan, lanes, pattern) in wrong.items():
        with pytest.raises(AssertionError, match=pattern) as ei:
            PM.check_plan(plan, m, lanes=lanes)
        messages[name] = str(ei.value)
    # five kinds of wrong plan, five kinds of message: none matches another's pattern
    for name, text in messages.items():
        assert [k for k, (_, _, pattern) in wrong.items() if re.search(pattern, text)] == [name]
    assert len(set(messages.values())) == 5
    for plan, lanes, pattern in ((order[:-1], None, "list 7 is missing"), (order, 7, "lane count 7, the model's is 8")):
        with pytest.raises(AssertionError, match=pattern):
            PM.check_plan(plan, m, lanes=lanes)
    # a big class out of order is a class error too: 2^14 sorts before 2^13
    with pytest.raises(AssertionError, match="class increases at position 1"):
        PM.check_plan([1, 5, 4, 8, 0, 6, 2, 7], m)
    # without an action list every list is a lane
    full = PM.plan_model(np.array([0, 64, 0], dtype=np.uint64), np.array([0, 1, 2, 3], dtype=np.uint64))
    PM.check_plan([1, 0, 2], full)
    with pytest.raises(AssertionError, match="list 2 is missing"):
        PM.check_plan([1, 0], full)
