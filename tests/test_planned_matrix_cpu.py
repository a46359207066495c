"""tests/planned_matrix.py checked without a GPU: its model against brute force and against
the library's host helpers (msha_alias_first, msha_blocks_for_len), every case against the
edge it is named for, so that none drifts off its path silently, and check_plan against
hand-damaged plans, one per property it states."""
import ctypes

import numpy as np
import pytest

import planned_matrix as M
from mirbft_amd import _lib as L
from mirbft_amd.engine import alias_first

U = np.uint64
T = M.T
CASES = M.cases()


def _tiles(n):
    return (n + T - 1) // T


def _edge_lens():
    """Every length at which blocks() or klass() changes, +- 1."""
    e = [0, 1, 55, 56, 63, 64, M.kFoldExactLen - 1, M.kFoldExactLen]
    for b in [M.kFoldLowBlocks, M.kFoldLowBlocks + 1, 4095, 4096, M.kLongBlocks] + [1 << k for k in range(12, 33)]:
        e += [(b - 2) * 64 + 55, (b - 2) * 64 + 56, (b - 1) * 64 + 55, (b - 1) * 64 + 56]   # b - 1 | b | b + 1 blocks
    out = sorted({max(x + d, 0) for x in e for d in (-1, 0, 1)})
    return np.array(out, dtype=U)


def test_constants_read_from_the_headers():
    assert (M.kPlanItems, M.kPlanTile, M.kGridGroups) == (16, 4096, 16)
    assert (M.kFoldExactLen, M.kFoldLowBlocks, M.kFoldBigBuckets, M.kLongBlocks) == (1024, 16, 52, 256)
    assert (M.kCoopMsgsPerWg, M.kChain2MsgsPerWg, M.kChain8MsgsPerWg) == (128, 64, 16)
    assert int(M.blocks(M.LONG_LEN)) == M.kLongBlocks and int(M.blocks(M.LONG_LEN - 9)) == M.kLongBlocks - 1
    assert int(M.blocks(M.BIG_LEN)) == 4096 and int(M.blocks(M.BIG_LEN - 1)) == 4095


def test_blocks_against_the_library():
    f = L.lib().msha_blocks_for_len
    lens = np.r_[_edge_lens(), np.random.default_rng(1).integers(0, 1 << 40, 2000).astype(U)]
    assert [int(x) for x in M.blocks(lens)] == [f(int(x)) for x in lens]


def test_klass_is_monotone_over_every_edge():
    lens = _edge_lens()
    c = M.klass(lens)
    assert (np.diff(c) >= 0).all()
    # and it steps exactly where the contract says: every length below kFoldExactLen, every
    # block count up to 4,096, every power of two above
    below = np.arange(M.kFoldExactLen + 1, dtype=U)
    assert (np.diff(M.klass(below)) > 0).all()
    step = lambda a, b: int(M.klass(U(b))) - int(M.klass(U(a)))   # noqa: E731
    for b in (18, 100, 4095, 4096):                       # b - 1 | b blocks
        assert step((b - 2) * 64 + 55, (b - 2) * 64 + 56) == 1, b
        assert step((b - 2) * 64 + 56, (b - 1) * 64 + 55) == 0, b
    for k in range(13, 33):
        b = 1 << k
        assert step((b - 2) * 64 + 55, (b - 2) * 64 + 56) == 1, k
        assert step((b - 2) * 64 + 56, (2 * b - 2) * 64 + 55) == 0, k
    assert int(M.klass(U(1023))) == 1023 and int(M.klass(U(1024))) == M.kFoldExactLen + 17 - M.kFoldLowBlocks
    assert int(M.klass(U((1 << 32) * 64))) < M.kFoldExactLen + 4096 - M.kFoldLowBlocks + M.kFoldBigBuckets


def test_case_names_are_distinct_and_counted():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    # the GPU test is parametrised by index over the nominal list: another CU count or
    # long_cap gives as many cases, in the same order
    other = M.cases(cus=304, long_cap=600)
    assert len(other) == len(CASES)
    assert [c.name.split("-")[0] for c in other] == [c.name.split("-")[0] for c in CASES]


def test_sizes():
    assert [_tiles(n) for n in M.sizes_lane()] == [1] * 9 + [2, 3, 16, 17, 34]
    for cus in (64, 256, 304):
        coop, head, many, steps = M.sizes_auto(cus)
        assert coop == cus * 128 and head == coop + 1
        assert _tiles(many) > max(cus, 64) and _tiles(many) % 64 == 44      # the gate's 64-workgroup grid
        assert _tiles(steps) >= 130 and _tiles(steps) % M.kGridGroups and steps > coop and steps % 16


def _local_fresh(off):
    """Above every earlier offset of its OWN tile (the insert's first pass)."""
    o = off.astype(np.int64)
    out = np.zeros(o.size, bool)
    for t0 in range(0, o.size, T):
        seg = o[t0:t0 + T]
        out[t0:t0 + T] = seg > np.r_[np.int64(-1), np.maximum.accumulate(seg)[:-1]]
    return out


@pytest.mark.parametrize("idx", [i for i, c in enumerate(CASES) if c.fold], ids=lambda i: CASES[i].name)
def test_case_model_and_edge(idx):
    c = CASES[idx]
    b = c.make()
    n, e = b.n, c.edge
    early_on = bool(c.expect.get("early_on", c.policy == "auto" and n > M.NOMINAL_CUS * 128))
    f = M.fresh(b.off, b.len, early_on)
    assert not (b.off % U(16)).any() and int((b.off + b.len).max()) <= b.arena_bytes
    # the library's host rule: a fresh message repeats nothing before it; among the others,
    # the first of each key (the one msha_alias_first names itself) is a lane: the count
    first = alias_first(b.off, b.len)
    assert (first[f] == np.flatnonzero(f)).all()
    cand = ~f
    lead = int((alias_first(b.off[cand], b.len[cand]) == np.arange(int(cand.sum()))).sum()) if cand.any() else 0
    lanes = M.model_lanes(b.off, b.len, early_on)
    assert lanes == int(f.sum()) + lead
    if n <= 2 * T + 1 or (n <= 33 * T + 5 and e.get("pattern") in ("backrefs", "straddle")):
        assert M.reference_fold(b.off, b.len, early_on) == lanes
    # the edge the case is named for
    if "n" in e:
        assert n == e["n"]
    p = e.get("pattern")
    if p == "rising":
        assert f.all() and lanes == n
    elif p == "one_payload":
        assert lanes == min(n, 2) and int(f.sum()) == 1      # message 0 and one claimant
    elif p == "falling":
        assert lanes == n and int(f.sum()) == 1
        if n >= 2 * T:
            assert (~f[T:2 * T]).all()                      # all 4,096 of a tile are candidates: 16 claim rounds
            assert T // 256 == 16
    elif p == "backrefs":
        if n > T:
            demoted = _local_fresh(b.off) & ~M.fresh(b.off, b.len, False)
            assert demoted[T:].any() and demoted[T]        # some message is demoted in the second pass
            assert lanes < n
    elif p == "never_fold":
        assert lanes == n and np.unique(M.keys(b.off, b.len)).size == n
        if n > 65:
            assert int(cand.sum()) >= n - n // 65 - 1
    elif p == "zero_len":
        assert not b.len.any() and lanes == min(n, 5) + min(max(n - 5, 0), 5)
    elif p == "straddle":
        if n > T + 1:
            k = M.keys(b.off, b.len)
            assert k[T - 1] == k[T] and cand[T - 1] and cand[T] and lanes < n
    if "margin" in e:
        assert e["margin"] >= 10, e                        # an order of magnitude inside the gate's inequality
        assert (M.blocks(b.len) >= M.kLongBlocks).sum() >= 2 and not f[M.blocks(b.len) >= M.kLongBlocks].any()
    if "longs" in e:
        long_keys = np.unique(M.keys(b.off, b.len)[M.blocks(b.len) >= M.kLongBlocks])
        assert long_keys.size == e["longs"] and (M.blocks(b.len) >= M.kLongBlocks).sum() == 2 * e["longs"]
        assert (M.blocks(b.len)[M.blocks(b.len) >= M.kLongBlocks] == M.kLongBlocks).all()
    if e.get("class_edges"):
        bl = set(int(x) for x in M.blocks(b.len))
        assert {16, 17, 18, 4095, 4096, 8191, 8192, M.kLongBlocks - 1, M.kLongBlocks} <= bl
        assert {1023, 1024} <= set(int(x) for x in b.len) and b.arena_bytes <= 32 * n + 16 + 600 * 1024
        long_keys, cnt = np.unique(M.keys(b.off, b.len)[b.len > U(64)], return_counts=True)
        assert (cnt == 3).all() and long_keys.size == 24


def test_early_list_cases_cover_the_capacity():
    names = [c.name for c in CASES if c.name.startswith("early-list-")]
    assert names == ["early-list-1", "early-list-cap-1", "early-list-cap", "early-list-cap+1"]
    last = [c for c in CASES if c.name == "early-list-cap+1"][0]
    assert last.expect["early"] == 0 and last.expect["long_listed"] == last.expect["long_cap"] + 1


def test_sequence_edges():
    s = M.sequence()
    a, b, c, d = (x.make() for x in s)
    assert (a.n, b.n, c.n, d.n) == (17 * T, 300, T + 1, 17 * T)
    assert np.array_equal(a.off[:300], b.off) and np.array_equal(a.len[:300], b.len)   # the same keys, a new epoch
    assert M.model_lanes(a.off, a.len, False) < a.n // 2                                # heavy aliasing
    assert [x.fold for x in s] == [True, True, False, True] and not s[2].wait and s[2].stream != s[3].stream


@pytest.mark.parametrize("name,make,shards", M.direct_cases(), ids=[c[0] for c in M.direct_cases()])
def test_direct_case_edges(name, make, shards):
    b = make()
    pieces, groups, bmax, B = M.direct_shape(b)
    keys = M.direct_keys(b)
    most = max(np.unique(keys[t0:t0 + T]).size for t0 in range(0, b.n, T))
    if make is M.direct_c:
        # B == 1, from the case's own numbers -- and on each of 3 shards too: a shard has at
        # least a quarter of the pieces (the split is by bytes; a third, less slack)
        assert B == 1 and groups * (bmax + 1) > M.DIRECT_BUCKETS
        assert 2 * (pieces // 4) * (bmax + 1) > M.DIRECT_BUCKETS
    else:
        assert B == bmax + 1 > 1
        assert most > 1024, most                           # the LDS key table of a tile is full
    assert (groups == 2 * pieces) == (make in (M.direct_c, M.direct_d))
    if make is M.direct_d:
        assert int((M.blocks(b.len) >= M.kLongBlocks).sum()) == 5
    if make is M.direct_b:
        f = M.fresh(b.off, b.len, False)
        assert 0.05 * b.n < (~f).sum() and M.model_lanes(b.off, b.len, False) < b.n
    assert b.n >= 3 * T and not (b.off % U(16)).any()


# --------------------------------------------------------------------------- check_plan bites

def _ideal(off, ln, fold, long_cap=0, head_cap=0, head_per_wg=64):
    """A plan the contract allows, built from the model: lanes by descending class."""
    n = len(off)
    f = M.fresh(off, ln, long_cap != 0) if fold else np.ones(n, bool)
    k = M.keys(off, ln)
    cand = np.flatnonzero(~f)
    _, first = np.unique(k[cand], return_index=True)
    lanes = np.sort(np.r_[np.flatnonzero(f), cand[first]])
    lanes = lanes[np.argsort(-M.klass(ln[lanes]), kind="stable")]
    order = np.full(n, M.NO_LANE, np.uint32)
    order[:lanes.size] = lanes
    nlong = int((M.blocks(ln[lanes]) >= M.kLongBlocks).sum()) if long_cap else 0
    plan = dict(n=n, folded=int(fold), lanes=lanes.size, head=nlong, early=nlong, late=0, long_lanes=nlong,
                long_listed=nlong, gate=int(nlong > 0), long_cap=long_cap, head_cap=head_cap,
                head_per_wg=head_per_wg, gave_up=0)
    return plan, order, order[:nlong][::-1].copy()


@pytest.fixture(scope="module")
def good():
    b = M._with_longs(M.p_mixed(3 * T + 9, 5), 3, 2, M.LONG_LEN, 5)
    ln = b.len.copy()
    ln[10], ln[11] = 1500, 9_000                         # more classes among the fresh lanes
    plan, order, longs = _ideal(b.off, ln, True, long_cap=8, head_cap=64)
    assert M.check_plan(b.off, ln, True, plan, order, longs) == []
    assert plan["early"] == 3 and plan["lanes"] < b.n - 100
    return b.off, ln, plan, order, longs


def _problems(good, plan=None, order=None, longs=None, **kw):
    off, ln, p, o, lg = good
    p = dict(p, **(plan or {}))
    return M.check_plan(off, ln, True, p, o if order is None else order, lg if longs is None else longs, **kw)


def test_good_plans_pass(good):
    off, ln, plan, order, longs = good
    assert _problems(good) == []
    # any order inside a class, and either claimant of a key, passes
    o = order.copy()
    c = M.klass(ln[o[:plan["lanes"]].astype(np.int64)])
    same = np.flatnonzero(c[:-1] == c[1:])
    p = int(same[same > plan["early"]][0])
    o[p], o[p + 1] = o[p + 1], o[p]
    assert _problems(good, order=o) == []
    k = M.keys(off, ln)
    f = M.fresh(off, ln, True)
    lanes = o[:plan["lanes"]].astype(np.int64)
    for q, i in enumerate(lanes):
        other = np.flatnonzero((k == k[i]) & ~f)
        if not f[i] and other.size > 1 and M.blocks(ln[i]) < M.kLongBlocks:
            o[q] = other[other != i][0]
            break
    else:
        raise AssertionError("no key with two candidates")
    assert _problems(good, order=o) == []
    # unfolded: a permutation by class
    plan2, order2, longs2 = _ideal(off, ln, False, head_cap=64)
    assert M.check_plan(off, ln, False, plan2, order2, longs2) == []
    assert M.check_plan(off, ln, False, dict(plan2, late=64, head=64), order2, longs2) == []


def test_two_lanes_swapped_across_a_class_are_reported(good):
    off, ln, plan, order, _ = good
    c = M.klass(ln[order[:plan["lanes"]].astype(np.int64)])
    p = int(np.flatnonzero(c[:-1] != c[1:])[-1])
    o = order.copy()
    o[p], o[p + 1] = o[p + 1], o[p]
    assert any("class rises" in x for x in _problems(good, order=o))


def test_a_doubled_lane_is_reported(good):
    o = good[3].copy()
    p = good[2]["lanes"] - 5
    o[p] = o[p + 1]
    assert any("listed twice" in x for x in _problems(good, order=o))


def test_no_lane_inside_the_lanes_is_reported(good):
    o = good[3].copy()
    o[good[2]["lanes"] // 2] = M.NO_LANE
    assert any("kNoLane inside the lanes" in x for x in _problems(good, order=o))


def test_a_tail_one_short_is_reported(good):
    off, ln, plan, order, _ = good
    lanes = plan["lanes"]
    folded = np.setdiff1d(np.arange(len(off)), order[:lanes].astype(np.int64))[0]
    o = order.copy()
    o[lanes] = folded                                     # a stale word where the tail begins
    assert any("past the lanes is not kNoLane" in x for x in _problems(good, order=o))
    # and a lane count one off, either way
    assert any("the model has" in x for x in _problems(good, plan={"lanes": lanes - 1}))
    assert any("the model has" in x for x in _problems(good, plan={"lanes": lanes + 1}, order=o))


def test_a_long_lane_missing_from_longs_is_reported(good):
    off, ln, plan, order, longs = good
    lg = longs.copy()
    lg[0] = order[plan["lanes"] - 1]
    assert any("early head's list" in x for x in _problems(good, longs=lg))
    # a long lane outside the head's positions
    o = order.copy()
    o[0], o[plan["early"]] = o[plan["early"]], o[0]
    assert any("exactly the long lanes" in x for x in _problems(good, order=o, longs=o[:plan["early"]].copy()))
    assert any("early 3, long_lanes 2" in x for x in _problems(good, plan={"long_lanes": 2}))
    assert any("early 3" in x for x in _problems(good, plan={"long_cap": 2}))


def test_wrong_lanes_are_reported(good):
    off, ln, plan, order, _ = good
    f = M.fresh(off, ln, True)
    lanes = order[:plan["lanes"]].astype(np.int64)
    o = order.copy()
    q = int(np.flatnonzero(f[lanes])[0])
    o[q] = np.setdiff1d(np.arange(len(off)), lanes)[0]    # a fresh message hashed by nobody
    assert any("fresh messages are lanes" in x for x in _problems(good, order=o))


def test_head_and_counters_are_reported(good):
    assert any("head 9" in x for x in _problems(good, plan={"head": 9}))
    assert any("head_cap" in x for x in _problems(good, plan={"head": 65, "early": 65, "head_cap": 64}))
    assert any("late head 5" in x for x in _problems(good, plan={"early": 0, "late": 5, "head": 5, "long_lanes": 0}))
    assert any("gave up" in x for x in _problems(good, plan={"gave_up": 2}))
    assert any("folded" in x for x in _problems(good, plan={"folded": 0}))
    assert any("forced to at least" in x for x in _problems(good, expect={"head_min": 4}))
    assert any("early = 3, expected 0" in x for x in _problems(good, expect={"early": 0}))
    assert _problems(good, expect={"early": 3, "head_min": 3, "early_on": True}) == []


def test_digests_helper_is_hashlib():
    import hashlib
    b = M.p_mixed(50, 3)
    a = b.arena()
    d = M.digests(a, b.off, b.len)
    for i in (0, 4, 9, 49):
        assert bytes(d[i]) == hashlib.sha256(a[int(b.off[i]):int(b.off[i] + b.len[i])].tobytes()).digest()
    assert ctypes.sizeof(L.MshaPlannedPlan) == 64
