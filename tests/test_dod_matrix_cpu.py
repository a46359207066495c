"""The digest-of-digests matrix (tests/dod_matrix.py) checked without a GPU: the
restated launch rules at their edges; per target and CU count, the cells its cases
reach against the cells its patterns promise (restated here from the patterns'
descriptions, so a thinned pattern fails here and not silently on the GPU); the
kernel every n gives; the size cap; and a model of what a lane hashes, run with one
seeded fault at a time, each of which must change a digest of some case."""
import hashlib

import numpy as np
import pytest

import dod_matrix as DM
import kernel_matrix as KM

CUS = (8, 64, 256, 304)
BIG = 256
KINDS = (DM.U_EVEN, DM.U_ODD, DM.NEAR0, DM.NEAR_OTHER, DM.RAGGED)
ALL_COUNT_CELLS = {(m, ge4, m == 0 and not ge4) for m in range(4) for ge4 in (False, True)}
ALL_SEGMENT_CELLS = {(-1, p, True) for p in (0, 1)} | {(s, p, False) for s in (0, 1) for p in (0, 1)}
EDGE_WHO = ("spread", "first", "middle", "last")


def test_restated_rules():
    """kernels.hip:1770-1785 (plan_split with the cap of 12), :716 (the stage) and
    host_entries.cpp msha_digest_of_digests (the small path), at their edges."""
    for c in CUS:
        S = 4 * c
        assert DM.plan_split(64 * S, c) is None and DM.plan_split(64 * (S - 1), c) is None
        assert DM.plan_split(64 * S + 1, c) == {"n_main": 64 * S, "chains": 1, "segments": 12, "groups": 8}
        assert DM.plan_split(64 * (S + S // 2), c)["segments"] == 2
        assert DM.plan_split(64 * (S + S // 2) + 1, c) is None
        assert DM.plan_split(64 * S + 1, c, "coop") is None
        sp = DM.plan_split(64 * (S + 33), c)
        if sp and sp["chains"] == 33:      # 33 chains: 9 workgroups of 4, rounded up to a multiple of 8
            assert sp["groups"] == 16 and sp["segments"] == min(12, S // 33)
        for tag, r_of, segs in DM.SPLIT_R:
            sp = DM.plan_split(DM.n_split(r_of)(c), c)
            assert sp and sp["chains"] == r_of(S) and sp["segments"] == segs, (tag, c, sp)
            assert sp["segments"] * sp["groups"] * 4 >= sp["chains"] * sp["segments"]
    assert DM.PER_LANE == 24 and DM.IDX_STAGE == 1536
    assert DM.is_staged(1536, 64) and not DM.is_staged(1537, 64)
    assert DM.is_staged(888, 37) and not DM.is_staged(889, 37)
    assert DM.host_small(65536, 32768) and not DM.host_small(65537, 0) and not DM.host_small(10, 32769)
    assert not DM.host_small(10, 10, small_bytes=0)
    assert DM.segment_bounds(13, 11, 12) == (11, 13) and DM.segment_bounds(1, 11, 12) == (0, 1)
    assert DM.segment_bounds(1, 0, 12) == (0, 0)


def test_shard_bounds_follow_the_block_midpoints():
    """host_plan.hpp partition() by its definition, brute force."""
    rng = np.random.default_rng(5)
    for _ in range(20):
        cnt = rng.integers(0, 40, int(rng.integers(1, 60)))
        k = int(rng.integers(2, 5))
        b = cnt // 2 + 1
        want = [0]
        for s in range(1, k):
            acc, hit = 0, len(cnt)
            for i, bi in enumerate(b):
                if 2 * k * acc + k * bi >= 2 * s * int(b.sum()):
                    hit = i
                    break
                acc += bi
            want.append(hit)
        assert DM.shard_bounds(cnt, k) == want + [len(cnt)]
    assert DM.shard_bounds(np.array([5, 0]), 3) == [0, 0, 1, 2]


# ---------------------------------------------------------------------------
# The promises, restated from the patterns' descriptions in plain integers
# ---------------------------------------------------------------------------
NEAR_PAIRS = [(0, 1), (0, 2), (1, 0), (1, 2), (1, 3), (2, 0), (2, 3), (2, 4), (20, 0), (20, 21), (20, 22),
              (21, 0), (21, 22), (21, 23), (24, 0), (24, 25), (24, 26)]       # (base, the odd lane's count)


def _edge_cell(act, d, who):
    """(staged, kind) of an edge wave: span 24 act + d, spread or held by one lane."""
    if who == "spread":
        return (d == 0, DM.U_EVEN if d == 0 else DM.NEAR_OTHER)
    return (d == 0, DM.NEAR0 if who == "first" else DM.NEAR_OTHER)


def _fill_cell(first_msg, lanes, mod, k):
    span = sum((i * 7919) % mod for i in range(first_msg, first_msg + lanes))
    return (span <= 24 * lanes, DM.RAGGED, lanes < 64, k % 4)


def promised_waves(pattern, m):
    """The wave cells of m lanes of DigestSrc::full under `pattern`."""
    W, tail = divmod(m, 64)
    cells = set()
    if pattern in ("uniform_up", "uniform_down"):
        for k in range(W):
            cnt = k % 34 if pattern == "uniform_up" else 33 - k % 34
            cells.add((cnt <= 24, DM.U_EVEN if cnt % 2 == 0 else DM.U_ODD, False, k % 4))
        if tail:
            cells.add((True, DM.U_EVEN, True, W % 4) if pattern == "uniform_up" else (False, DM.U_ODD, True, W % 4))
        return cells
    if pattern.startswith("ragged"):
        start = 12 if pattern == "ragged12" else 0
        return {_fill_cell(start + 64 * k, 64 if k < W else tail, 48, k) for k in range(W + (tail > 0))}
    if pattern.startswith("near_uniform_l"):
        lane = int(pattern[14:])
        designed = [(63 * b + o <= 1536, DM.NEAR0 if lane == 0 else DM.NEAR_OTHER) for b, o in NEAR_PAIRS]
        tail_cell = {0: (True, DM.U_ODD), 1: (False, DM.U_EVEN)}.get(lane)      # 37 x 23 = 851, 37 x 26 = 962
    else:
        assert pattern.startswith("stage_edges")
        designed = [_edge_cell(64, d, who) for who in EDGE_WHO for d in (0, 1)]
        tail_cell = None
        if pattern != "stage_edges":
            p = int(pattern[13:])
            tail_cell = _edge_cell(37, p % 2, EDGE_WHO[p // 2])
    for k in range(W):
        cells.add(designed[k] + (False, k % 4) if k < len(designed) else _fill_cell(64 * k, 64, 16, k))
    if tail:
        cells.add(tail_cell + (True, W % 4) if tail_cell else _fill_cell(64 * W, tail, 16, W))
    return cells


def _single_launch_targets():
    return [t for t in DM.targets() if t["kernel"] in ("dod", "split")]


def _union(t, c):
    waves, edges, counts, segs = set(), set(), set(), set()
    for p in sorted({p for p, _ in t["cases"]}):
        w, e, k, s = DM.case_cells(t, p, c)
        waves |= w
        edges |= e
        counts |= k
        segs |= s
    return waves, edges, counts, segs


@pytest.mark.parametrize("c", CUS)
@pytest.mark.parametrize("name", [t["name"] for t in _single_launch_targets()])
def test_cells_reached_equal_cells_promised(name, c):
    t = DM.target(name)
    waves, edges, counts, segs = _union(t, c)
    want = set()
    for p in {p for p, _ in t["cases"]}:
        n = DM.n_of(t, p, c)
        sp = DM.plan_split(n, c, t["policy"])
        if p == "over_limit":       # ragged, its last message grown to reach 32,769 indices
            want |= promised_waves("ragged", n - 37) | {(False, DM.RAGGED, True, (n // 64) % 4)}
        else:
            want |= promised_waves(p, sp["n_main"] if sp else n)
    assert waves == want, (sorted(waves - want), sorted(want - waves))
    if t["kernel"] == "split":
        assert segs == ALL_SEGMENT_CELLS, sorted(ALL_SEGMENT_CELLS - segs)
    else:
        assert segs == set()


def _minimum(waves, partial_too):
    paths = {(st, kind, part) for st, kind, part, _ in waves}
    want = {(st, kind, part) for st in (True, False) for kind in KINDS for part in ((False, True) if partial_too
                                                                                    else (False,))}
    assert want <= paths, sorted(want - paths)
    for st in (True, False):
        assert {slot for s, _, _, slot in waves if s == st} == {0, 1, 2, 3}, st


@pytest.mark.parametrize("c", CUS)
def test_unsplit_target_reaches_the_minimum(c):
    """All five final-block kinds, staged and direct, in full and in partial waves;
    both paths in all four wave slots; both stage edges at 64 and at 37 lanes, spread
    and held by the first, a middle and the last lane; every count cell."""
    waves, edges, counts, _ = _union(DM.target("dod_device"), c)
    _minimum(waves, partial_too=True)
    assert edges == {(act, d, who) for act in (64, 37) for d in (0, 1) for who in EDGE_WHO}
    assert counts == ALL_COUNT_CELLS


@pytest.mark.parametrize("c", CUS)
@pytest.mark.parametrize("tag", [s[0] for s in DM.SPLIT_R])
def test_split_targets_reach_the_minimum(tag, c):
    """The main workgroups (full waves only): every kind on both paths, every slot,
    both edges at 64 lanes, every count cell; the surplus lanes every segment cell."""
    t = DM.target("dod_split_" + tag)
    waves, edges, counts, segs = _union(t, c)
    assert not any(part for _, _, part, _ in waves)
    _minimum(waves, partial_too=False)
    assert edges == {(64, d, who) for d in (0, 1) for who in EDGE_WHO}
    assert counts == ALL_COUNT_CELLS and segs == ALL_SEGMENT_CELLS
    main = DM.plan_split(t["n"](c), c)["n_main"]
    up = DM.case_begin(t, "uniform_up", c)
    down = DM.case_begin(t, "uniform_down", c)
    present = set(DM._counts(up, main).tolist()) | set(DM._counts(down, main).tolist())
    assert present == set(range(34))                                  # every count 0..33 in a uniform wave
    assert {DM.count_cell(v) for v in range(34)} == ALL_COUNT_CELLS


def test_count_cells_are_the_eight():
    assert len(ALL_COUNT_CELLS) == 8 and {DM.count_cell(v) for v in (0, 1, 2, 3, 4, 5, 6, 7)} == ALL_COUNT_CELLS
    # what whole launches of the counts 0, 1, 2, 3, 20, 21, 40 and 1000 leave out
    assert ALL_COUNT_CELLS - {DM.count_cell(v) for v in (0, 1, 2, 3, 20, 21, 40, 1000)} \
        == {(2, True, False), (3, True, False)}


def test_near_uniform_waves_are_as_described():
    for lane in DM.NEAR_LANES:
        combos = DM.near_combos(lane)
        assert [(b, o) for b, _, o in combos] == NEAR_PAIRS
        cnt = DM.near_uniform(64 * 20, lane)
        for w, (b, j, o) in enumerate(combos):
            wave = cnt[64 * w:64 * w + 64]
            assert j == lane and wave[j] == o and (np.delete(wave, j) == b).all()
    assert (20, 22) in NEAR_PAIRS                                       # even counts that differ
    first_direct = [p for p in NEAR_PAIRS if 63 * p[0] + p[1] > 1536][0]
    assert first_direct == (24, 25)


def test_thinned_pattern_fails_the_coverage_check():
    """The check has teeth: without its near-uniform waves for lane 0 the unsplit
    target misses the lane-0 cells."""
    t = DM.target("dod_device")
    waves = set()
    for p in {p for p, _ in t["cases"]} - {"near_uniform_l0"} - {"stage_edges_p%d" % k for k in (2, 3)}:
        waves |= DM.case_cells(t, p, BIG)[0]
    with pytest.raises(AssertionError):
        _minimum(waves, partial_too=True)


# ---------------------------------------------------------------------------
# Kernel choice, the sharded batches, the size cap
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", CUS)
def test_every_n_gives_the_kernel_its_target_claims(c):
    seen = set()
    for t in DM.targets():
        for p in {p for p, _ in t["cases"]}:
            n = DM.n_of(t, p, c)
            assert DM.expected_kernel(t, p, c) == t["kernel"], (t["name"], p, c, n)
            assert n == 2 or p == "zero_runs" or n % 64 == DM.PARTIAL_LANES, (t["name"], p, n)
            d = DM.expected_deltas(t, p, c)
            assert set(d) == set(DM.COUNTERS)
            if t["kernel"] == "dod":
                assert d == KM._only(launches_dod=1, small_calls=0)
            elif t["kernel"] == "split":
                assert d == KM._only(launches_split=1, launches_dod=0, small_calls=0)
            elif t["kernel"] == "small":
                assert d["small_calls"] == 1 and d["launches_dod"] == 0 and d["launches_split"] == 0
                assert sum(d[k] for k in ("launches_lane", "launches_pipe", "launches_coop")) == 1
        seen.add(t["kernel"])
    assert seen == {"dod", "split", "small", "shards"}
    assert DM.plan_split(DM.N_UNSPLIT, c) is None
    # the policy target's n would split under auto
    t = DM.target("dod_device_coop_policy")
    assert DM.plan_split(t["n"](c), c, "auto") and not DM.plan_split(t["n"](c), c, "coop")


def test_small_path_limit_sits_on_its_edge():
    small, over = DM.target("dod_host_small"), DM.target("dod_host_over_limit")
    assert int(DM.case_begin(small, "limit", BIG)[-1]) == 32768
    assert int(DM.case_begin(over, "over_limit", BIG)[-1]) == 32769
    assert over["env"] == {}                                           # MSHA_SMALL_BYTES untouched


@pytest.mark.parametrize("c", CUS)
def test_sharded_batches(c):
    t = DM.target("dod_host_sharded")
    assert DM.shards_of(t) == 3 and t["fresh"]
    # so few messages that a shard is empty
    ls = DM.launches(t, "two", c)
    assert [(lo, hi) for lo, hi, _ in ls] == [(0, 1), (1, 2)]
    assert DM.expected_deltas(t, "two", c) == KM._only(launches_dod=2, small_calls=0)
    # both boundaries inside a run of empty messages; the later shards start past index 0
    cnt = DM.case_counts(t, "zero_runs", c)
    b = DM.shard_bounds(cnt, 3)
    for cut in b[1:3]:
        assert (cnt[cut - 50:cut + 50] == 0).all(), cut
    begin = DM.case_begin(t, "zero_runs", c)
    assert 0 < begin[b[1]] < begin[b[2]] < begin[-1]
    # the ragged one: three shards, none empty, cut inside waves
    ls = DM.launches(t, "ragged", c)
    assert len(ls) == 3 and all(lo % 64 for lo, _, _ in ls[1:])
    for p in ("ragged", "zero_runs"):
        d = DM.expected_deltas(t, p, c)
        assert d["launches_dod"] + d["launches_split"] == 3 and d["small_calls"] == 0
        assert d["launches_split"] == sum(1 for _, _, sp in DM.launches(t, p, c) if sp)


def test_size_cap():
    """A condition, not a measurement: on 256 CUs no case hands the oracle more than
    64 MiB of table rows, and no target has more than 40 cases."""
    worst = 0
    for t in DM.targets():
        assert len(t["cases"]) <= 40 and len(set(t["cases"])) == len(t["cases"]), t["name"]
        for p in {p for p, _ in t["cases"]}:
            worst = max(worst, DM.table_bytes(t, p, BIG))
            assert DM.table_bytes(t, p, BIG) <= 64 << 20, (t["name"], p, DM.table_bytes(t, p, BIG))
            assert DM.n_of(t, p, BIG) <= 2 * 1024 * 64 + 64
    assert worst > 32 << 20         # and the large cases are large: direct waves by the thousand
    assert max(DM.n_of(t, p, BIG) for t in DM.targets() for p, _ in t["cases"] if "x2" not in t["name"]) == 98277
    assert len(DM.cases()) == sum(len(t["cases"]) for t in DM.targets())


def test_index_patterns():
    for ip in DM.INDEX_PATTERNS:
        table, idx = DM.build_index(ip, 5000, 77)
        assert len(idx) == 5000 and idx.dtype == np.uint32 and int(idx.max()) < len(table)
        assert len({r.tobytes() for r in table}) == len(table)         # rows pairwise distinct
        t0, i0 = DM.build_index(ip, 0, 77)
        assert len(i0) == 0 and len(t0) >= 1
    table, idx = DM.build_index("contiguous", 5000, 1)
    assert (idx == np.arange(5000)).all() and len(table) == 5000
    table, idx = DM.build_index("random", 50000, 1)
    assert len(table) == 4099 and (idx[1:] != idx[:-1]).all() and len(np.unique(idx)) > 4000
    table, idx = DM.build_index("one_row", 10, 1)
    assert len(table) == 4099 and (idx == 4098).all()
    table, idx = DM.build_index("table1", 10, 1)
    assert len(table) == 1 and (idx == 0).all()


# ---------------------------------------------------------------------------
# Sensitivity: a model of what a lane hashes, with one seeded fault at a time
# ---------------------------------------------------------------------------
STALE = b"\xee" * 32        # what a lane gets where nothing it should read was put

FAULTS = ("stage_base", "stage_cap_plus", "stage_cap_minus", "uniform_ignores_lane0", "uniform_if_all_even",
          "drop_odd", "bits_cnt0", "skip_two", "b0_ceil", "no_rebase")


def _final(row, cnt):
    """kernels.hip:614-632 dod_final_words."""
    head = (row + b"\x80" + bytes(23)) if row is not None else (b"\x80" + bytes(55))
    return head + (256 * cnt).to_bytes(8, "big")


def _lane_stream(rd, cnt, uniform, pad_cnt, cnt0, fault):
    """kernels.hip:659-693 DigestSrc::digest: the 64-byte blocks one lane compresses."""
    out, k = [], 0
    while k + 4 <= cnt:
        out += [rd(k), rd(k + 1), rd(k + 2), rd(k + 3)]
        k += 4
    if k + 2 <= cnt and fault != "skip_two":
        out += [rd(k), rd(k + 1)]
        k += 2
    if uniform:
        out.append(_final(None, pad_cnt))
    else:
        one = k < cnt and fault != "drop_odd"
        out.append(_final(rd(k) if one else None, cnt0 if fault == "bits_cnt0" else cnt))
    return b"".join(out)


def _model_launch(b, rows, m, sp, fault):
    """The block streams of one launch's m messages: b its begin, rows the table rows
    of its idx, joined. Lanes below n_main (all, unsplit) as DigestSrc::full, the
    surplus lanes as the split chains' segments."""
    def row(k):
        return rows[32 * k:32 * k + 32] if 0 <= k and 32 * k + 32 <= len(rows) else STALE

    out = []
    full = sp["n_main"] if sp else m
    for w0 in range(0, full, 64):
        w1 = min(w0 + 64, full)
        act, s0 = w1 - w0, int(b[w0])
        span = int(b[w1]) - s0
        staged = span <= 24 * act + (fault == "stage_cap_plus")
        copied = min(span, 24 * act - (fault == "stage_cap_minus"))
        cnts = [int(b[i + 1] - b[i]) for i in range(w0, w1)]
        cnt0 = cnts[0]
        if fault == "uniform_ignores_lane0" and act > 1:
            pad_cnt = cnts[1]
            uniform = all(v == pad_cnt for v in cnts[1:]) and pad_cnt % 2 == 0
        elif fault == "uniform_if_all_even":
            pad_cnt, uniform = cnt0, all(v % 2 == 0 for v in cnts)
        else:
            pad_cnt, uniform = cnt0, all(v == cnt0 for v in cnts) and cnt0 % 2 == 0
        for i in range(w0, w1):
            k0 = int(b[i])
            if staged:
                base = 0 if fault == "stage_base" else k0 - s0

                def rd(k, base=base):
                    return row(s0 + base + k) if base + k < copied else STALE
            else:
                def rd(k, k0=k0):
                    return row(k0 + k)
            out.append(_lane_stream(rd, cnts[i - w0], uniform, pad_cnt, cnt0, fault))
    for i in range(full, m):        # kernels.hip:744-766, 797-798
        k0, cnt = int(b[i]), int(b[i + 1] - b[i])
        nb, segs, blocks = cnt // 2 + 1, sp["segments"], []
        for seg in range(segs):
            b0, b1 = DM.segment_bounds(nb, seg, segs)
            if fault == "b0_ceil":
                b0 = -(-nb * seg // segs)
            for blk in range(b0, b1):
                if blk < cnt // 2:
                    blocks.append(row(k0 + 2 * blk) + row(k0 + 2 * blk + 1))
                else:
                    one = 2 * blk < cnt and fault != "drop_odd"
                    blocks.append(_final(row(k0 + 2 * blk) if one else None, cnt))
        out.append(b"".join(blocks))
    return out


def model(t, pattern, index_pattern, c, fault=None):
    """The block streams of a case's messages (host_entries.cpp msha_digest_of_digests: every shard gets
    idx + i0 and begin - i0)."""
    begin = DM.case_begin(t, pattern, c).astype(np.int64)
    table, idx = DM.build_index(index_pattern, int(begin[-1]), KM._salt(t["name"], pattern, index_pattern))
    out = []
    for lo, hi, sp in DM.launches(t, pattern, c):
        i0 = int(begin[lo])
        rows = table[idx[i0:]].tobytes()
        b = begin[lo:hi + 1] - (0 if fault == "no_rebase" else i0)
        out += _model_launch(b, rows, hi - lo, sp, fault)
    return out, table, idx, begin


def _padded(msg):
    return msg + b"\x80" + bytes((55 - len(msg)) % 64) + (8 * len(msg)).to_bytes(8, "big")


SMALL_C = 8
_T = {t["name"]: t for t in DM.targets()}
# the cases that launch the kernel, the smallest first (a fault is looked for until a case notices it)
MODEL_CASES = sorted([(t, p, ip) for t, p, ip in DM.cases() if _T[t]["kernel"] != "small"],
                     key=lambda case: DM.n_of(_T[case[0]], case[1], SMALL_C))


def test_the_model_without_a_fault_hashes_what_sha256_hashes():
    """Every lane's block stream is its joined rows, padded as FIPS 180-4 says: so
    the model's digests are the expected ones."""
    large = (("dod_device", "stage_edges_p1", "contiguous"), ("dod_device", "near_uniform_l0", "one_row"),
             ("dod_host_pipeline", "uniform_up", "random"))
    assert set(large) <= set(MODEL_CASES)
    for name, p, ip in MODEL_CASES:
        t = DM.target(name)
        if DM.n_of(t, p, SMALL_C) > 5000 and (name, p, ip) not in large:
            continue        # 16 K messages a case: three of them here
        streams, table, idx, begin = model(t, p, ip, SMALL_C)
        rows = table[idx].tobytes()
        exp = DM.expected_hashlib(table, idx, begin.astype(np.uint64))
        assert len(streams) == len(begin) - 1
        for i, s in enumerate(streams):
            msg = rows[32 * begin[i]:32 * begin[i + 1]]
            assert s == _padded(msg), (name, p, ip, i)
            assert hashlib.sha256(msg).digest() == exp[i].tobytes()


@pytest.mark.parametrize("fault", FAULTS)
def test_every_seeded_fault_changes_a_digest(fault):
    """As tests/test_parts_plan_matrix_cpu.py shows that check_plan rejects each kind
    of wrong plan: each fault in the model changes the block stream (so the digest) of
    at least one message of at least one case."""
    caught = None
    for name, p, ip in MODEL_CASES:
        t = DM.target(name)
        if fault == "b0_ceil" and t["kernel"] != "split":
            continue
        if fault == "no_rebase" and t["kernel"] != "shards":
            continue
        good = model(t, p, ip, SMALL_C)[0]
        bad = model(t, p, ip, SMALL_C, fault)[0]
        diff = [i for i, (g, b) in enumerate(zip(good, bad)) if g != b]
        if diff:
            caught = (name, p, ip, len(diff))
            break
    assert caught, "no case of the matrix notices the fault %r" % fault


def test_the_edge_faults_are_caught_only_on_the_edge():
    """The two stage-capacity faults leave every wave correct but those with a span
    of exactly 24 act (+ 1), and spoil each of those: stage_edges' eight, the
    uniform wave of count 24, near_uniform's 63 x 24 with one 25."""
    t = DM.target("dod_split_r1")
    main = DM.plan_split(t["n"](SMALL_C), SMALL_C)["n_main"]
    for fault, delta in (("stage_cap_plus", 1), ("stage_cap_minus", 0)):
        for p, ip in t["cases"]:
            good, _, _, begin = model(t, p, ip, SMALL_C)
            bad = model(t, p, ip, SMALL_C, fault)[0]
            diff = {i // 64 for i, (g, b) in enumerate(zip(good, bad)) if g != b}
            on_edge = {w for w in range(main // 64) if int(begin[64 * w + 64] - begin[64 * w]) == 1536 + delta}
            assert diff == on_edge, (fault, p, sorted(diff)[:5])
            if p == "stage_edges":      # spread, first, middle, last
                assert diff == {w for w, (d, _) in enumerate(DM.EDGE_FORMS) if d == delta}
            if p == "ragged":
                assert not diff


# ---------------------------------------------------------------------------
# The expected values, the report, the guard
# ---------------------------------------------------------------------------
def test_oracle_agrees_with_hashlib_on_the_small_cases():
    pytest.importorskip("oracle")
    from oracle import oracle
    done = 0
    for name, p, ip in DM.cases():
        t = DM.target(name)
        if DM.n_of(t, p, SMALL_C) > DM.HASHLIB_MAX:
            continue
        begin = DM.case_begin(t, p, SMALL_C)
        table, idx = DM.build_index(ip, int(begin[-1]), KM._salt(name, p, ip))
        assert np.array_equal(oracle.digest_of_digests(table, idx, begin), DM.expected_hashlib(table, idx, begin)), \
            (name, p, ip)
        done += 1
    assert done >= 40


def test_expected_switches_to_the_oracle_above_hashlib_max(monkeypatch):
    """Up to HASHLIB_MAX messages hashlib alone computes the expected digests; one
    message more and the oracle does, and its rows agree with hashlib's."""
    pytest.importorskip("oracle")
    from oracle import oracle
    calls = []
    real = oracle.digest_of_digests
    monkeypatch.setattr(oracle, "digest_of_digests", lambda *a: calls.append(len(a[2]) - 1) or real(*a))
    for n in (DM.HASHLIB_MAX, DM.HASHLIB_MAX + 1):
        begin = DM.to_begin(DM.ragged(n))
        table, idx = DM.build_index("random", int(begin[-1]), 3)
        got = DM.expected(table, idx, begin)
        assert got.shape == (n, 32) and got[0].tobytes() == hashlib.sha256(b"").digest()
        for i in (1, 47, 48, n - 1):
            rows = table[idx[int(begin[i]):int(begin[i + 1])]].tobytes()
            assert got[i].tobytes() == hashlib.sha256(rows).digest(), (n, i)
    assert calls == [DM.HASHLIB_MAX + 1]


def test_mismatch_report_names_wave_lane_count_and_path():
    t = DM.target("dod_split_r1")
    begin = DM.case_begin(t, "stage_edges", SMALL_C)
    ls = DM.launches(t, "stage_edges", SMALL_C, begin)
    exp = np.zeros((len(begin) - 1, 32), np.uint8)
    got = exp.copy()
    assert DM.mismatch("x", begin, got, exp, ls) is None
    got[64 * 3 + 0, 1] = 1          # wave 3: one more than the stage holds, all in lane 0
    got[64 * 9 + 5, 0] = 1          # a filler wave
    got[32 * 64 + 3, 0] = 1         # a surplus chain's lane
    m = DM.mismatch("x", begin, got, exp, ls)
    assert m["bad"] == 3 and m["what"] == "x"
    assert m["first"][0] == {"message": 192, "count": 1537, "path": "direct", "shard": 0, "wave": 3, "lane": 0,
                             "wave_kind": "near-uniform (lane 0 odd)"}
    assert m["first"][1]["path"] == "staged" and m["first"][1]["wave_kind"] == "ragged" and m["first"][1]["lane"] == 5
    assert m["first"][2]["path"] == "chain lane" and m["first"][2]["segments"] == 12 and m["first"][2]["count"] == 3


def test_kernel_matrix_has_no_digest_of_digests_target():
    """The guard: the day tests/kernel_matrix.py gains a digest-of-digests target,
    merge the two matrices instead of keeping two sets of launch rules."""
    src = open(KM.__file__).read()
    assert "launches_dod" not in src and "digest_of_digests" not in src and \
        not any("dod" in t["name"] or "dod" in t["entry"] for t in KM.targets()), \
        "tests/kernel_matrix.py now names the digest-of-digests kernel: merge tests/dod_matrix.py into it"
