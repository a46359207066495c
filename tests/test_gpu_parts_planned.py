"""msha_hash_actions_device_planned on the GPU (mirbft_amd/csrc/parts_plan.hip): multi-part
actions named through part lists, folded (a list is hashed once however many actions
name it, an unnamed one not at all) and ordered by descending block-count class inside
the call. Every expected digest is hashlib's of the joined parts or a committed fixture
(tests/golden/actions.json), never another path of the engine. Shapes are the smallest
at which the planner can go wrong: more than three waves, lists on both sides of the
wave-sum threshold, zero-part lists, every block-count class next to a different one."""
import hashlib
import os
import re

import numpy as np
import pytest

import parts_matrix
import parts_plan_matrix
from mirbft_amd import MshaError, pack_parts
from mirbft_amd import _lib as L

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLACK = L.MSHA_DEVICE_ARENA_SLACK
CAPTURE_MESSAGE = "make one call of this size outside the capture first"


def _wave_sum_threshold() -> int:
    """T: lists of T parts or more are summed by a whole wave (parts_plan.hpp)."""
    text = open(os.path.join(ROOT, "mirbft_amd", "csrc", "parts_plan.hpp")).read()
    return int(re.search(r"constexpr uint32_t kWaveSumParts = (\d+);", text).group(1))


def _sha(parts) -> bytes:
    return hashlib.sha256(b"".join(parts)).digest()


def _want(actions) -> np.ndarray:
    return np.frombuffer(b"".join(_sha(a) for a in actions), dtype=np.uint8).reshape(-1, 32)


def _blocks(nbytes: int) -> int:
    return nbytes // 64 + (1 if nbytes % 64 < 56 else 2)


def _dev(a: np.ndarray):
    import torch
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.size == 0:
        return torch.empty(0, dtype=torch.from_numpy(a).dtype, device="cuda:0")
    return torch.from_numpy(a).to("cuda:0")


def _call(engine, arena, off, ln, begin, action_list=None):
    """One hash_actions_device_planned call on uploaded copies -> the out tensor (0xA5-filled before)."""
    import torch
    n = begin.size - 1 if action_list is None else action_list.size
    out = torch.full((n, 32), 0xA5, dtype=torch.uint8, device="cuda:0")
    engine.hash_actions_device_planned(_dev(arena), _dev(off), _dev(ln), _dev(begin), out,
                                       action_list=None if action_list is None else _dev(action_list))
    return out


def _run(engine, arena, off, ln, begin, action_list=None) -> np.ndarray:
    out = _call(engine, arena, off, ln, begin, action_list)
    engine.device_status()
    return out.cpu().numpy()


def _packed(lists):
    """pack_parts(): parts back to back, hence unaligned; the device contract's slack appended."""
    arena, off, ln, begin = pack_parts(lists)
    return np.concatenate([arena, np.full(SLACK, 0xEE, dtype=np.uint8)]), off, ln, begin


def _bad_rows(got, want):
    return [int(i) for i in np.nonzero((got != want).any(axis=1))[0]]


def _cut(rng, msg: bytes, k: int):
    cuts = sorted(int(c) for c in rng.integers(0, len(msg) + 1, size=k - 1))
    edges = [0] + cuts + [len(msg)]
    return [msg[a:b] for a, b in zip(edges, edges[1:])]


@gpu
def test_boundary_matrix_without_action_list(engine):
    """tests/parts_matrix.py's batch (L = 0..200 in 0..6 parts, both sides of every
    padding and block edge cut in two at every position, all start residues), action i
    = list i: one call, four workgroups, block counts 1..4 mixed."""
    arena, off, ln, begin, want, seen = parts_matrix.boundary_matrix()
    assert seen == set(range(16))
    got = _run(engine, arena, off, ln, begin)
    bad = _bad_rows(got, want)
    assert bad == [], (len(bad), bad[:8])
    order = engine.parts_plan_order()
    assert sorted(order.tolist()) == list(range(begin.size - 1))


@gpu
def test_mixed_classes_in_one_call(engine):
    """204 lists (more than three waves) of 1, 2, 3, 9, 17 and 70 blocks in index order
    that mixes them, a 5,000-byte one-part list, a zero-part list, and lists of T - 1, T
    and T + 1 one-byte parts around the wave-sum threshold T (the first summed by its
    lane, the others by the wave; in one wave with short lists). The digests are right,
    the order is a permutation of the lists, and block counts never increase along it."""
    T = _wave_sum_threshold()
    rng = np.random.default_rng(0x9C)
    sizes = {1: 10, 2: 64, 3: 130, 9: 512, 17: 1024, 70: 4420}
    assert all(_blocks(v) == k for k, v in sizes.items())
    lists = []
    for i in range(198):
        nbytes = list(sizes.values())[(i * 5 + i // 6) % 6]
        lists.append(_cut(rng, rng.bytes(nbytes), 1 + i % 4))
    lists.insert(17, [rng.bytes(5000)])
    lists.insert(70, [])
    for at, k in ((3, T - 1), (4, T), (130, T + 1), (131, 2 * T + 64 + 1)):
        lists.insert(at, [rng.bytes(1) for _ in range(k)])
    assert len(lists) == 204
    arena, off, ln, begin = _packed(lists)
    got = _run(engine, arena, off, ln, begin)
    assert _bad_rows(got, _want(lists)) == []
    order = engine.parts_plan_order()
    assert sorted(order.tolist()) == list(range(len(lists)))
    parts_plan_matrix.check_plan(order, parts_plan_matrix.plan_model(ln, begin))
    blocks = np.array([_blocks(sum(len(p) for p in a)) for a in lists])
    along = blocks[order]
    assert (np.diff(along) <= 0).all(), along.tolist()
    assert {1, 2, 3, 9, 17, 70, 79} <= set(along.tolist())


@gpu
def test_folding_hashes_each_named_list_once(engine, actions_golden, monkeypatch):
    """40 lists, 1,000 actions: list 7 named 300 times, lists 3, 11, 19 and 33 never,
    the golden EpochChange (1,505 parts) among the named. Digests are right per action;
    under MSHA_PARTS_TIMING=1 last_lanes is the number of distinct named lists and
    last_blocks their block sum; the order holds exactly the named lists, the EpochChange first."""
    ec = next(parts for name, kind, parts, _ in actions_golden if kind == "epoch_change" and len(parts) > 1000)
    rng = np.random.default_rng(0xF0)
    lists = [_cut(rng, rng.bytes(int(rng.integers(0, 700))), 1 + i % 5) for i in range(40)]
    lists[22] = ec
    unnamed = {3, 11, 19, 33}
    named = [l for l in range(40) if l not in unnamed]
    al = np.array([named[int(x)] for x in rng.integers(0, len(named), 1000)], dtype=np.uint32)
    al[:len(named)] = named                      # every named list at least once
    al[len(named) + rng.choice(1000 - len(named), 300, replace=False)] = 7
    assert (al == 7).sum() >= 300 and set(al.tolist()) == set(named)
    arena, off, ln, begin = _packed(lists)
    want = _want(lists)[al]
    monkeypatch.setenv("MSHA_PARTS_TIMING", "1")
    got = _run(engine, arena, off, ln, begin, action_list=al)
    st = engine.parts_plan_stats()
    monkeypatch.delenv("MSHA_PARTS_TIMING")
    assert _bad_rows(got, want) == []
    assert st["last_lanes"] == len(named)
    assert st["last_blocks"] == sum(_blocks(sum(len(p) for p in lists[l])) for l in named)
    assert st["last_kernel_ms"] > 0
    order = engine.parts_plan_order()
    assert sorted(order.tolist()) == named and order[0] == 22
    parts_plan_matrix.check_plan(order, parts_plan_matrix.plan_model(ln, begin, al), lanes=st["last_lanes"])
    # without the variable nothing is read back
    got = _run(engine, arena, off, ln, begin, action_list=al)
    st = engine.parts_plan_stats()
    assert _bad_rows(got, want) == []
    assert (st["last_lanes"], st["last_blocks"], st["last_kernel_ms"]) == (0, 0, 0.0)


@gpu
def test_unnamed_lists_are_not_dereferenced(engine):
    """A list no action names may have any part range: here the unnamed lists' ranges
    lie beyond the part arrays, and one of them decreases."""
    rng = np.random.default_rng(0xDE)
    a, b = [rng.bytes(77), rng.bytes(3)], [rng.bytes(200)]
    arena, off, ln, _ = _packed([a, b])
    begin = np.array([0, 2, 3, 1 << 40, 0], dtype=np.uint64)     # lists 0: a, 1: b, 2 and 3: never named
    al = np.array([1, 0, 0, 1], dtype=np.uint32)
    got = _run(engine, arena, off, ln, begin, action_list=al)
    assert _bad_rows(got, _want([b, a, a, b])) == []
    assert sorted(engine.parts_plan_order().tolist()) == [0, 1]


@gpu
def test_errors_are_flagged_and_zeroed(engine):
    """One action_list entry out of range and one list with a decreasing part range in
    an otherwise good call: that action and every action naming that list get all-zero
    digests, all others are right, device_status() raises MSHA_ERR_INVALID_ARG once and
    is clean afterwards. Every offset stays inside the arena. Then each error alone, for
    its message, and the host-side refusals."""
    import torch
    rng = np.random.default_rng(0xE7)
    lists = [[rng.bytes(int(rng.integers(1, 90))) for _ in range(3)] for _ in range(20)]
    arena, off, ln, begin = _packed(lists)
    # every boundary twice: list 2k = [begin[k], begin[k+1]) is the real list k, list 2k+1 is empty
    pairs = np.concatenate([np.repeat(begin, 2)[1:-1], begin[-1:]]).astype(np.uint64)
    assert pairs.size == 41 and pairs[18] == begin[9] and pairs[19] == begin[10] == pairs[20]
    pairs[19] = pairs[18] - np.uint64(2)         # list 18 (real list 9) decreases; list 19 gains five parts, in bounds
    n_lists = pairs.size - 1
    al = (2 * rng.integers(0, 20, 300)).astype(np.uint32)
    al[[5, 50, 299]] = 18
    al[123] = n_lists                                            # out of range by one
    real = list(lists)
    want = _want(real)[np.minimum(al // 2, 19)]
    zero = sorted(set(np.nonzero(al == 18)[0].tolist()) | {123})
    # list 19 (the gap after real list 9) now runs from begin[19] to pairs[20]: a real, in-bounds range
    assert not (al == 19).any()
    out = _call(engine, arena, off, ln, pairs, action_list=al)
    with pytest.raises(MshaError) as ei:
        engine.device_status()
    assert ei.value.code == L.MSHA_ERR_INVALID_ARG
    assert "action_part_begin decreases" in str(ei.value) and "action_list out of range" in str(ei.value)
    engine.device_status()                      # reported once, then clean
    got = out.cpu().numpy()
    assert not got[zero].any()
    assert _bad_rows(got, want) == zero
    # the out-of-range id alone
    al2 = al.copy()
    al2[al2 == 18] = 0
    out = _call(engine, arena, off, ln, pairs, action_list=al2)
    with pytest.raises(MshaError) as ei:
        engine.device_status()
    assert ei.value.code == L.MSHA_ERR_INVALID_ARG and "action_list out of range" in str(ei.value)
    assert "decreases" not in str(ei.value)
    engine.device_status()
    got = out.cpu().numpy()
    assert not got[123].any() and _bad_rows(got, _want(real)[np.minimum(al2 // 2, 19)]) == [123]
    # a good call afterwards is exact
    assert _bad_rows(_run(engine, arena, off, ln, begin), _want(lists)) == []
    # host-side refusals, each with a context: an unknown flag, counts that disagree
    d = [_dev(x) for x in (arena, off, ln, begin)]
    o = torch.zeros((20, 32), dtype=torch.uint8, device="cuda:0")
    lib, ctx = engine._lib, engine._ctx
    args = [t.data_ptr() for t in d]
    assert lib.msha_hash_actions_device_planned(ctx, *args, 20, None, 20, 2, o.data_ptr(), None) == L.MSHA_ERR_INVALID_ARG
    assert b"unknown flags" in lib.msha_last_error(ctx)
    assert lib.msha_hash_actions_device_planned(ctx, *args, 20, None, 19, 0, o.data_ptr(), None) == L.MSHA_ERR_INVALID_ARG
    assert b"must equal n_lists" in lib.msha_last_error(ctx)
    assert lib.msha_hash_actions_device_planned(ctx, *args, 20, None, 20, L.MSHA_PARTS_FOLD, o.data_ptr(), None) == L.MSHA_OK
    assert lib.msha_hash_actions_device_planned(ctx, *args, 20, _dev(al).data_ptr(), 0, 0, o.data_ptr(), None) == L.MSHA_OK
    engine.device_status()
    assert _bad_rows(o.cpu().numpy(), _want(lists)) == []


@gpu
def test_golden_actions_named_in_reverse(engine, actions_golden):
    """Every golden action as a list; the actions name them last to first, and the
    digests land in action order."""
    lists = [parts for _, _, parts, _ in actions_golden]
    n = len(lists)
    want = np.frombuffer(b"".join(d for _, _, _, d in actions_golden), dtype=np.uint8).reshape(-1, 32)
    al = np.arange(n, dtype=np.uint32)[::-1].copy()
    got = _run(engine, *_packed(lists), action_list=al)
    bad = _bad_rows(got, want[::-1])
    assert bad == [], [actions_golden[n - 1 - i][0] for i in bad]
    got = _run(engine, *_packed(lists))
    assert _bad_rows(got, want) == []


@gpu
@pytest.mark.parametrize("with_list", [False, True], ids=["direct", "action_list"])
def test_capturable_into_a_graph(engine, with_list):
    """After one warm call of the same size the call captures into a HIP graph (a linear
    chain of kernels on the caller's stream; nothing runs during the
    capture), and each replay hashes what the arena holds by then."""
    import torch
    rng = np.random.default_rng(0x6B)
    lists = [[rng.bytes(int(rng.integers(0, 300))) for _ in range(int(rng.integers(0, 5)))] for _ in range(300)]
    arena, off, ln, begin = _packed(lists)
    al = rng.integers(0, 300, 500).astype(np.uint32) if with_list else None
    n = 500 if with_list else 300
    d_arena, d_off, d_ln, d_begin = _dev(arena), _dev(off), _dev(ln), _dev(begin)
    d_al = _dev(al) if with_list else None
    out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda:0")
    engine.hash_actions_device_planned(d_arena, d_off, d_ln, d_begin, out, action_list=d_al)     # the warm call
    engine.device_status()
    out.zero_()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            engine.hash_actions_device_planned(d_arena, d_off, d_ln, d_begin, out, action_list=d_al, stream=s)
        finally:
            g.capture_end()
    torch.cuda.synchronize()
    assert not out.any()
    for seed in (1, 2):
        fresh = np.random.default_rng(seed).integers(0, 256, arena.size, dtype=np.uint8)
        d_arena.copy_(_dev(fresh))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        engine.device_status()
        host = fresh.tobytes()
        want = _want([[host[int(off[j]):int(off[j] + ln[j])] for j in range(int(begin[i]), int(begin[i + 1]))]
                      for i in range(300)])
        if with_list:
            want = want[al]
        assert _bad_rows(out.cpu().numpy(), want) == [], seed


@gpu
def test_capture_without_a_warm_call_fails_cleanly():
    """A fresh context has no workspace and may not allocate one while the stream is
    being captured: MSHA_ERR_INVALID_ARG and the documented message, the capture ends
    empty, and the same call outside capture then works."""
    import torch
    from mirbft_amd import Engine
    rng = np.random.default_rng(0x6C)
    lists = [[rng.bytes(40), rng.bytes(41)] for _ in range(70)]
    arena, off, ln, begin = _packed(lists)
    d = [_dev(x) for x in (arena, off, ln, begin)]
    out = torch.zeros((70, 32), dtype=torch.uint8, device="cuda:0")
    with Engine(1) as eng:
        s = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.capture_begin()
            try:
                with pytest.raises(MshaError) as ei:
                    eng.hash_actions_device_planned(*d, out, stream=s)
            finally:
                g.capture_end()
        torch.cuda.synchronize()
        assert ei.value.code == L.MSHA_ERR_INVALID_ARG and CAPTURE_MESSAGE in str(ei.value)
        assert not out.any()
        eng.hash_actions_device_planned(*d, out)
        eng.device_status()
        assert _bad_rows(out.cpu().numpy(), _want(lists)) == []


@gpu
def test_counters_are_separate(engine):
    """The new entry counts in msha_parts_plan_stats alone: parts_stats() and
    stats()["planned_device_calls"] do not move; hash_actions_device leaves
    parts_plan_stats() alone."""
    import torch
    rng = np.random.default_rng(6)
    lists = [[rng.bytes(10), rng.bytes(9)] for _ in range(70)]
    arena, off, ln, begin = _packed(lists)
    al = np.array([5, 5, 69], dtype=np.uint32)
    p0, s0, q0 = engine.parts_stats(), engine.stats(), engine.parts_plan_stats()
    assert _bad_rows(_run(engine, arena, off, ln, begin), _want(lists)) == []
    assert _bad_rows(_run(engine, arena, off, ln, begin, action_list=al), _want(lists)[al]) == []
    p1, s1, q1 = engine.parts_stats(), engine.stats(), engine.parts_plan_stats()
    assert p1 == p0 and s1 == s0
    assert q1["calls"] - q0["calls"] == 2 and q1["actions"] - q0["actions"] == 73
    assert q1["lists"] - q0["lists"] == 140
    assert q1["launches_plan"] - q0["launches_plan"] == 4 + 5        # init, measure, scan, scatter; and mark
    assert q1["launches_hash"] - q0["launches_hash"] == 2 and q1["launches_fill"] - q0["launches_fill"] == 1
    assert (q1["last_lanes"], q1["last_blocks"], q1["last_kernel_ms"]) == (0, 0, 0.0)
    out = torch.zeros((70, 32), dtype=torch.uint8, device="cuda:0")
    engine.hash_actions_device(_dev(arena), _dev(off), _dev(ln), _dev(begin), out)
    engine.device_status()
    assert engine.parts_plan_stats() == q1
    assert engine.parts_stats()["calls"] == p1["calls"] + 1
