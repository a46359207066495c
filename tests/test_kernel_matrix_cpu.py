"""The kernel matrix (tests/kernel_matrix.py) checked without a GPU: every batch
size stays inside the range of the kernel it is aimed at, by the launchers'
thresholds restated from mirbft_amd/csrc/kernels.hip; every target x pattern hits,
by its lengths alone, each cell it promises (so a thinned pattern fails here, not
silently on the GPU); and the expected digests -- the oracle's scalar FIPS 180-4
leg -- agree with hashlib on the patterns' full inputs."""
import hashlib

import numpy as np
import pytest

import kernel_matrix as KM

BIG, SMALL = 256, 8        # CUs: the MI355X's count, and one where S/2 + 3 is small
LEN_CELLS = {KM.len_cell(L) for L in range(384)}   # every (r class, nfull mod 4, nfull == 0)


def test_len_cells_are_the_fifteen():
    # three r classes x (nfull == 0, and nfull mod 4 = 0..3 with nfull > 0)
    assert len(LEN_CELLS) == 15


def test_restated_thresholds():
    """The few lines of kernels.hip the range checks rest on, at their edges:
    pick_mode (kPipe up to one wave per SIMD, kPair from three), uses_coop (128
    messages a CU), plan_split (q >= 1 full rounds, surplus 0 < r <= SIMDs / 2) and
    launch_digest_batch's chain8 / chain2 / coop ladder (16 / 64 / 128 a CU)."""
    c = BIG
    assert KM.pick_mode(c * 256, c) == 3 and KM.pick_mode(c * 256 + 1, c) == 1
    assert KM.pick_mode(c * 768 - 1, c) == 1 and KM.pick_mode(c * 768, c) == 2
    assert KM.pick_mode(10, c, forced=0) == 0 and KM.pick_mode(10 ** 7, c, forced=3) == 3
    assert KM.uses_coop(c * 128, c, "auto") and not KM.uses_coop(c * 128 + 1, c, "auto")
    assert KM.uses_coop(10 ** 7, c, "coop") and not KM.uses_coop(1, c, "lane")
    S = 4 * c
    assert KM.plan_split(64 * S, c, "auto") is None                       # r == 0
    assert KM.plan_split(64 * S + 1, c, "auto") == (64 * S, 1)
    assert KM.plan_split(64 * (S + S // 2), c, "lane") == (64 * S, S // 2)
    assert KM.plan_split(64 * (S + S // 2) + 1, c, "auto") is None        # r > S / 2
    assert KM.plan_split(64 * (S - 1), c, "auto") is None                 # q == 0
    assert KM.plan_split(64 * S + 1, c, "coop") is None
    assert KM.batch_kernel(16 * c, c) == ("chain8", 1) and KM.batch_kernel(16 * c + 1, c) == ("chain2", 1)
    assert KM.batch_kernel(16 * c, c, small8=False) == ("chain2", 1)
    assert KM.batch_kernel(64 * c + 1, c) == ("coop", 1) and KM.batch_kernel(128 * c + 1, c) == ("pipe", 3)
    assert KM.batch_kernel(64 * (3 * S + 5), c) == ("split", 2) and KM.batch_kernel(64 * (S + 5), c) == ("split", 1)
    assert KM.batch_kernel(64 * (S + 5), c, forced=3) == ("split", 1)     # split_mode honours 0..2 only
    assert KM.batch_kernel(64 * (S + 5), c, forced=0) == ("split", 0)


@pytest.mark.parametrize("cus", [BIG, SMALL])
def test_every_n_inside_its_kernels_range(cus):
    seen = set()
    for t in KM.targets():
        if t["fixed_n"] and cus != BIG:
            continue    # 64 x 300 is a size for the MI355X's 1,024 SIMDs, not a function of S
        n = t["n"](cus)
        assert KM.expected_kernel(t, cus) == KM.target_kernel(t), (t["name"], cus, n, KM.expected_kernel(t, cus))
        if t["entry"] != "batch" or not t["per_wg"]:
            assert n % 64 == KM.PARTIAL_LANES, (t["name"], n)            # a partial last wave of 37
        else:
            assert t["name"] == "coop_policy" or n % t["per_wg"] == t["per_wg"] - 5   # a partial last workgroup
        seen.add(KM.target_kernel(t))
    # every kernel and load mode the matrix names is reached by some target
    want = {("lane", 1), ("lane", 2), ("lane_ws", 1), ("split", 1), ("chain8", 1), ("chain2", 1), ("coop", 1)}
    assert want <= seen and (cus != BIG or ("pipe", 3) in seen)


def test_forced_mode_child_ranges():
    """The child process' shapes on 256 CUs: the forced mode decides on the small
    shape (no split, no cooperative kernel under policy lane), and the split shape
    splits with modes 0 to 2 honoured."""
    for mode in range(4):
        small = ("pipe", 3) if mode == 3 else ("lane", mode)
        for case in KM.child_cases():
            want = ("split", mode if mode < 3 else 1) if case == "split" else small
            assert KM.child_expected(case, mode, BIG) == want, (case, mode)
    assert KM.plan_split(KM.CHILD_N, BIG, "lane") is None
    assert len(KM.child_cases()) == 4 + 14 + 1
    assert {int(c.split("len")[1].split("_")[0]) for c in KM.child_cases() if c.startswith("uniform_len")} \
        == set(KM.UNIFORM_LENS)


# ---------------------------------------------------------------------------
# Coverage: the cells each pattern promises, restated here from the matrix's
# description and not from the generator's code.
# ---------------------------------------------------------------------------
def _near_promise():
    cells = set()
    for L in (0, 56, 63, 64, 120, 128, 192):
        odd = {L + 64, 0}
        odd |= {L - 1} if L in (56, 64, 120, 128, 192) else set()    # across 55|56 or 63|64, downward
        odd |= {L + 1} if L == 63 else set()                         # across 63|64, upward
        odd.discard(L)
        assert len(odd) == (1 if L == 0 else 3)
        for kind in (KM.NEAR0, KM.NEAR_OTHER):
            cells.add(KM.len_cell(L) + (kind, False))
            cells |= {KM.len_cell(o) + (kind, False) for o in odd}
    return cells


def _promised(pattern):
    if pattern == "uniform64":
        return {c + (KM.UNIFORM, False) for c in LEN_CELLS} | {KM.len_cell(64) + (KM.UNIFORM, True)}
    if pattern == "uniform56":
        return {c + (KM.UNIFORM, False) for c in LEN_CELLS} | {KM.len_cell(56) + (KM.UNIFORM, True)}
    if pattern == "ragged":
        return {c + (KM.RAGGED, False) for c in LEN_CELLS}
    if pattern == "near_uniform":
        return _near_promise()
    raise KeyError(pattern)


def _missing(pattern, lens):
    return sorted(_promised(pattern) - KM.lane_cells(lens))


LANE_CASES = [(t, p) for t, p in KM.cases() if p in KM.LANE_PATTERNS]


@pytest.mark.parametrize("name,pattern", LANE_CASES, ids=["%s-%s" % c for c in LANE_CASES])
def test_lane_pattern_cells(name, pattern):
    t = KM.target(name)
    lens = KM.pattern_lengths(t, pattern, BIG)
    assert len(lens) == t["n"](BIG)
    kinds = KM.wave_kinds(lens)
    if pattern == "ragged":
        assert set(kinds) == {KM.RAGGED}                             # no wave is uniform
        assert any(c[3] == KM.RAGGED and c[4] for c in KM.lane_cells(lens))   # a ragged partial wave
    if pattern.startswith("uniform"):
        assert set(kinds) == {KM.UNIFORM}
    if pattern == "near_uniform":
        combos = KM.near_combos()
        assert len(combos) == 19 * 4 and kinds[:len(combos)].count(KM.NEAR0) == 19
        assert kinds[:len(combos)].count(KM.NEAR_OTHER) == 19 * 3
        assert set(kinds[len(combos):]) == {KM.RAGGED}
        for w, (L, j, o) in enumerate(combos):                      # exactly one odd lane, where promised
            wave = lens[64 * w:64 * w + 64]
            assert wave[j] == o and (np.delete(wave, j) == L).all(), (L, j, o)
    assert not _missing(pattern, lens), _missing(pattern, lens)


def test_thinned_pattern_fails_the_coverage_check():
    """The check has teeth: near_uniform without its lane-0 waves misses cells."""
    t = KM.target("lane_prefetch")
    lens = KM.near_uniform(t["n"](BIG))
    for w, (L, j, o) in enumerate(KM.near_combos()):
        if j == 0:
            lens[64 * w:64 * w + 64] = KM.ragged(64, start=64 * w)
    missing = _missing("near_uniform", lens)
    assert missing and all(c[3] == KM.NEAR0 for c in missing)


def test_child_uniform_variants_cover_lens_between_them():
    """At 300 waves neither uniform variant holds all 384 lengths; the upward and the
    downward walk together do, and each has its partial wave."""
    up, down = KM.child_lengths("uniform64", KM.CHILD_N), KM.child_lengths("uniform56", KM.CHILD_N)
    assert set(KM.wave_kinds(up)) == set(KM.wave_kinds(down)) == {KM.UNIFORM}
    assert set(up[:-37].tolist()) | set(down[:-37].tolist()) == set(range(384))
    cells = KM.lane_cells(up) | KM.lane_cells(down)
    assert not (_promised("uniform64") | _promised("uniform56")) - cells
    for p in ("near_uniform", "ragged"):
        assert not _missing(p, KM.child_lengths(p, KM.CHILD_N))


@pytest.mark.parametrize("name", [t["name"] for t in KM.targets() if t["entry"] == "planned"][:1])
@pytest.mark.parametrize("pattern,lengths", [("planned_uniform", KM.PLANNED_UNIFORM), ("planned_r0", KM.PLANNED_R0)])
def test_planned_pattern_cells(name, pattern, lengths):
    """The planner orders lanes by class, descending; below 1,024 B a class is one
    exact length (kernels.hpp kFoldExactLen). Sorted so, each length of the set owns
    whole waves (thousands of messages), and the class boundaries are mixed waves."""
    t = KM.target(name)
    lens = KM.pattern_lengths(t, pattern, BIG)
    assert sorted(set(KM.blocks(np.array(lengths)).tolist())) == list(range(1, len(lengths) + 1))
    assert all(L % 64 == 0 or L % 64 >= 56 for L in lengths)        # every length on the uniform-pad path
    counts = {L: int((lens == L).sum()) for L in lengths}
    assert min(counts.values()) >= 3000, counts
    cells = KM.lane_cells(np.sort(lens)[::-1])
    assert {KM.len_cell(L) + (KM.UNIFORM, False) for L in lengths} <= cells
    assert any(c[3] != KM.UNIFORM for c in cells)
    assert set(KM.wave_kinds(lens)) == {KM.RAGGED}                   # the input order itself is interleaved


def test_uniform_layout_cells():
    lens = {L for g in KM.UNIFORM_GROUPS.values() for L, _ in g}
    assert lens == set(KM.UNIFORM_LENS)
    for g in KM.UNIFORM_GROUPS.values():
        for L, stride in g:
            assert stride % 16 == 0 and stride >= max(16, (L + 15) // 16 * 16)
    assert (120, 256) in KM.UNIFORM_GROUPS["le192"]                  # one stride larger than needed
    # the r classes at nfull 0..3, and both uniform-pad cases (r == 0, r >= 56) with and without full blocks
    cells = {KM.len_cell(L) for L in lens}
    assert {(0, 0, True), (1, 0, True), (2, 0, True), (0, 1, False), (1, 1, False), (2, 1, False),
            (0, 2, False), (1, 2, False), (0, 3, False)} <= cells


PAIR_TARGETS = [t["name"] for t in KM.targets() if t["per_wg"]]


@pytest.mark.parametrize("name", PAIR_TARGETS)
def test_pair_pattern_cells(name):
    """(NB parity, NB < / == / > 64, a shorter message in the workgroup, length-only
    last block): each NB in {1, 62..66, 127..129} alone in its workgroup, in both
    spellings from 62 on; and every parity and side of the threshold again with
    1-block messages beside it."""
    t = KM.target(name)
    per = t["per_wg"]
    same = KM.pattern_lengths(t, "pair_same", BIG)
    mixed = KM.pattern_lengths(t, "pair_mixed", BIG)
    nb = KM.blocks(same)
    wgs = [set(nb[s:s + per].tolist()) for s in range(0, len(same), per)]
    assert all(len(w) == 1 for w in wgs)                              # each workgroup one nb
    assert {next(iter(w)) for w in wgs} == set(KM.PAIR_NB)
    want = {(1, -1, False, False)}
    for NB in KM.PAIR_NB[1:]:
        want |= {(NB % 2, (NB > 64) - (NB < 64), False, lo) for lo in (False, True)}
    assert want <= KM.pair_cells(same, per), sorted(want - KM.pair_cells(same, per))
    nbm = KM.blocks(mixed)
    for s in range(0, len(mixed) - per + 1, per):                     # every full workgroup mixes the three
        w = set(nbm[s:s + per].tolist())
        assert 1 in w and any(b % 2 and b > 1 for b in w) and any(b % 2 == 0 for b in w), (s, w)
    wantm = {(p, c, True, lo) for p, c in ((1, -1), (0, 0), (1, 1), (0, 1)) for lo in (False, True)}
    assert wantm <= KM.pair_cells(mixed, per), sorted(wantm - KM.pair_cells(mixed, per))
    # both spellings of the 64-block message, as the matrix names them
    assert {63 * 64, 62 * 64 + 60} <= set(same.tolist())


# ---------------------------------------------------------------------------
# The expected values themselves: the oracle against hashlib, on the full inputs.
# ---------------------------------------------------------------------------
def _oracle_vs_hashlib(arena, off, lens):
    got = KM.expected(arena, off, lens)
    buf = arena.tobytes()
    for i in range(len(lens)):
        o, l = int(off[i]), int(lens[i])
        assert got[i].tobytes() == hashlib.sha256(buf[o:o + l]).digest(), (i, o, l)


@pytest.mark.parametrize("pattern", KM.CHILD_PATTERNS)
def test_oracle_against_hashlib_lane_patterns(pattern):
    arena, off, lens = KM.build_arena(KM.child_lengths(pattern, KM.CHILD_N), 8 * 11)
    assert (off % 16 == 0).all() and len(arena) == int(off[-1]) + (int(lens[-1]) + 15) // 16 * 16 + 64
    _oracle_vs_hashlib(arena, off, lens)


@pytest.mark.parametrize("pattern,lengths", [("planned_uniform", KM.PLANNED_UNIFORM), ("planned_r0", KM.PLANNED_R0)])
def test_oracle_against_hashlib_planned_patterns(pattern, lengths):
    arena, off, lens = KM.build_arena(KM.planned_classes(KM.CHILD_N, lengths), 8 * 13, min_stride=16)
    assert len(set(off.tolist())) == len(off)                        # distinct offsets: nothing folds
    _oracle_vs_hashlib(arena, off, lens)


@pytest.mark.parametrize("mixed", [False, True])
def test_oracle_against_hashlib_pair_edges(mixed):
    t = KM.target("chain8")
    arena, off, lens = KM.build_arena(KM.pair_edges(t["n"](BIG), 16, mixed), 8 * 17)
    _oracle_vs_hashlib(arena, off, lens)


def test_oracle_against_hashlib_uniform_layout():
    for g in KM.UNIFORM_GROUPS.values():
        for msg_len, stride in g:
            _oracle_vs_hashlib(*KM.uniform_arena(msg_len, stride, 64 * 8 - 27, 8 * (msg_len + stride)))


def test_mismatch_report_names_wave_lane_length_and_kind():
    lens = KM.near_uniform(64 * 100 - 27)
    exp = np.zeros((len(lens), 32), np.uint8)
    got = exp.copy()
    assert KM.mismatch("t / p", lens, got, exp) is None
    got[64 * 4 + 0, 3] = 1      # wave 4 = (56, lane 0, odd 0): the odd lane itself
    got[64 * 80 + 5, 0] = 1
    m = KM.mismatch("t / p", lens, got, exp)
    assert m["bad"] == 2 and m["what"] == "t / p"
    assert m["first"][0] == {"message": 256, "wave": 4, "lane": 0, "len": 0, "blocks": 1,
                             "wave_kind": "near-uniform (lane 0 odd)"}
    assert m["first"][1]["wave_kind"] == "ragged" and m["first"][1]["lane"] == 5
