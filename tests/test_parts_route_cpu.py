"""The route model of msha_hash_actions_device_routed (tests/parts_route_matrix.py): the
builders proven to reach what they claim, by set equality; every "all fit" case shown
to fit its caps under the model alone; check_route() shown to reject wrong routes; and
the claim arithmetic of mirbft_amd/csrc/parts_route.hpp under AddressSanitizer + UBSan as
a stand-alone program with its own main (tests/cpp/parts_route_check.cpp). Host code
only: nothing is loaded into Python."""
import os
import re
import subprocess

import parts_route_matrix as M
from mirbft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mirbft_amd", "csrc")


def _counts(begin):
    return [int(b) - int(a) for a, b in zip(begin, begin[1:])]


def test_constants_are_the_sources():
    assert M.SLACK == L.MSHA_DEVICE_ARENA_SLACK
    assert M.DEFAULT_LONG_BLOCKS == L.MSHA_ROUTE_LONG_BLOCKS_DEFAULT
    assert M.DEFAULT_LONG_BYTES == L.MSHA_ROUTE_LONG_BYTES_DEFAULT
    text = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert int(re.search(r"constexpr unsigned kChain8MsgsPerWg = (\d+);", text).group(1)) == 16
    text = open(os.path.join(CSRC, "parts_plan.hpp")).read()
    assert int(re.search(r"constexpr uint32_t kExactBlocks = (\d+);", text).group(1)) == M.EXACT


def test_threshold_edge_covers_what_it_claims():
    case, (once, often, never) = M.threshold_edge()
    m = M.model_of(case)
    assert case.long_blocks == 4
    assert {n % 64 for n in M.EDGE_LENGTHS} == {55, 56, 0}
    for group in (once, often):
        assert [m.nbytes[l] for l in group] == list(M.EDGE_LENGTHS)
        assert sorted({m.blocks[l] for l in group}) == [2, 3, 4, 5]
    al = case.action_list.tolist()
    assert {al.count(l) for l in once} == {1} and {al.count(l) for l in often} == {M.EDGE_REPEAT}
    assert not set(never) & set(al) and not set(never) & m.named
    for l in never:                                                 # long by their parts, and unreadable
        b, e = int(case.begin[l]), int(case.begin[l + 1])
        assert M.blocks_for_bytes(int(case.part_len[b:e].sum())) in (2, 3, 4, 5)
        assert (case.part_off[b:e] >= M.FAR).all() and case.lists[l] is None
    assert m.long == {l for l in once + often if m.blocks[l] >= 4} and len(m.long) == 10
    # on the threshold: 183 bytes is 3 blocks, 184 is 4
    assert M.blocks_for_bytes(183) == 3 and M.blocks_for_bytes(184) == 4 and M.blocks_for_bytes(192) == 4
    assert m.all_fit and m.count == 10
    assert max(int(o + n) for o, n in zip(case.part_off, case.part_len) if o < M.FAR) + M.SLACK <= case.arena.size


def test_summing_paths_cover_what_they_claim():
    case, (three, many) = M.summing_paths()
    m = M.model_of(case)
    counts = _counts(case.begin)
    assert counts[three] == 3 and counts[many] == 300
    j = int(case.begin[three]) + 1
    assert int(case.part_len[j]) == 2000 and int(case.part_off[j]) % 2 == 1
    lens = case.part_len[int(case.begin[many]): int(case.begin[many + 1])]
    assert int(lens.max()) <= 40 and int((lens == 0).sum()) == 18 and {int(x) for x in lens if x} <= set(range(1, 41))
    text = open(os.path.join(CSRC, "parts_plan.hpp")).read()
    T = int(re.search(r"constexpr uint32_t kWaveSumParts = (\d+);", text).group(1))
    text = open(os.path.join(CSRC, "parts_concat.hpp")).read()
    step = int(re.search(r"constexpr uint32_t kStepParts = (\d+);", text).group(1))
    large = int(re.search(r"constexpr uint32_t kLargePart = (\d+);", text).group(1))
    assert counts[three] < T <= counts[many] and counts[many] > step and 2000 >= large
    assert m.long == {three, many} and m.all_fit


def test_one_wave_of_long_covers_what_it_claims():
    case = M.one_wave_of_long()
    m = M.model_of(case)
    assert m.long == set(range(3, 73)) and set(_counts(case.begin)[3:]) == {33}
    assert len({m.nbytes[l] for l in m.long}) == 5 and m.all_fit and m.count == 70
    assert 3 // 64 == 66 // 64 - 1 == 0                             # lists 3..66 share the first wave


def test_caps_cases():
    r16 = M.round16(M.CAP_LEN)
    assert r16 == 1008 and M.blocks_for_bytes(M.CAP_LEN) == 16
    for max_long, long_bytes, want, fit in ((2, 0, 2, False), (0, 3 * r16 + M.SLACK, 3, False),
                                            (0, 3 * r16 + M.SLACK - 1, 2, False), (1, 0, 1, False),
                                            (0, 0, 5, True), (4, 2 * r16 + M.SLACK + 15, 2, False),
                                            (5, 5 * r16 + M.SLACK, 5, True)):
        m = M.model_of(M.caps(max_long, long_bytes))
        assert len(m.long) == 5 and {m.nbytes[l] for l in m.long} == {M.CAP_LEN}
        assert (m.count, m.all_fit) == (want, fit), (max_long, long_bytes)


def test_uniform_and_mixed_cases():
    for n in (64, 65, 257):
        for with_list in (False, True):
            none, every = M.model_of(M.uniform(n, False, with_list)), M.model_of(M.uniform(n, True, with_list))
            assert none.named == every.named == set(range(n))
            assert none.long == set() and none.all_fit and none.count == 0
            assert every.long == set(range(n)) and every.all_fit and every.count == n
            assert {every.blocks[l] for l in range(n)} == {2}
    case, longs = M.mixed_batch()
    m = M.model_of(case)
    assert case.action_list.size == 4096 and m.long == set(longs) and len(longs) == 5 and m.all_fit
    counts = _counts(case.begin)
    assert {1, 20} <= set(counts) and max(m.blocks[l] for l in longs) == M.blocks_for_bytes(96000) == 1501


def test_empty_long_case():
    case = M.empty_long()
    m = M.model_of(case)
    assert case.long_blocks == 1 and m.named == {0, 1, 2, 4, 5, 6, 7} and m.long == m.named and m.all_fit
    assert [m.nbytes[l] for l in (1, 2, 5)] == [0, 0, 0] and _counts(case.begin)[1:3] == [0, 1]
    assert _counts(case.begin)[5] == 3 and {m.blocks[l] for l in (1, 2, 5)} == {1}
    want = M.expected_digests(case)
    import hashlib
    empty = hashlib.sha256(b"").digest()
    assert [i for i in range(9) if want[i].tobytes() == empty] == [1, 2, 4, 7, 8]
    # an empty list takes no room: the routed bytes are the other four lists'
    assert sum(M.round16(m.nbytes[l]) for l in m.long) == 16 + 64 + 64 + 208


def test_decreasing_long_case():
    case = M.decreasing_long()
    m = M.model_of(case)
    assert int(case.begin[3]) < int(case.begin[2]) and 2 in m.named and 2 not in m.valid
    between = int(case.part_len[int(case.begin[3]): int(case.begin[2])].sum())
    assert M.blocks_for_bytes(between) >= case.long_blocks          # long by the parts between its bounds
    assert m.long == {1, 3, 4} and 5 in case.action_list.tolist() and m.n_lists == 5
    want = M.expected_digests(case)
    assert not want[[2, 5, 6]].any() and want[[0, 1, 3, 4, 7]].any(axis=1).all()


def _fixture():
    case = M.caps(0, 0)
    m = M.model_of(case)
    long = sorted(m.long)
    short = sorted(m.named - m.long)
    nbytes = sum(M.round16(m.nbytes[l]) for l in long)
    return case, m, long, short, nbytes


def test_check_route_accepts_the_right_route():
    case, m, long, short, nbytes = _fixture()
    assert M.check_route(long, nbytes, sorted(short, key=lambda l: -m.cls[l]), m) == []
    # under a slot cap any two of the five will do
    m2 = M.model_of(M.caps(2, 0))
    lanes = sorted(set(m2.named) - {long[1], long[4]}, key=lambda l: -m2.cls[l])
    assert M.check_route([long[4], long[1]], 2 * 1008, lanes, m2) == []


def test_check_route_rejects_wrong_routes():
    case, m, long, short, nbytes = _fixture()
    lanes = sorted(short, key=lambda l: -m.cls[l])

    def problems(ids, b, order, model=m):
        return " | ".join(M.check_route(ids, b, order, model))

    assert "is routed and is not long" in problems(long + [short[0]], nbytes, [l for l in lanes if l != short[0]])
    assert "is routed and a lane" in problems(long, nbytes, [long[0]] + lanes)
    assert "is neither routed nor a lane" in problems(long[1:], nbytes - 1008, lanes)
    assert "routed twice" in problems(long + long[:1], nbytes, lanes)
    assert "routed_bytes" in problems(long, nbytes + 16, lanes)
    assert "class increases" in problems(long, nbytes, lanes[::-1])
    # an unnamed list routed
    edge, (once, often, never) = M.threshold_edge()
    me = M.model_of(edge)
    good_lanes = sorted(me.named - me.long, key=lambda l: -me.cls[l])
    assert M.check_route(sorted(me.long), sum(M.round16(me.nbytes[l]) for l in me.long), good_lanes, me) == []
    assert "no action names it" in problems(sorted(me.long) + [never[5]], 0, good_lanes, me)
    assert "is a lane and no action names it" in problems(sorted(me.long), 0, good_lanes + [never[0]], me)
    # a count over max_long, bytes over long_bytes, a count that is not the header's
    m2 = M.model_of(M.caps(2, 0))
    rest = sorted(m2.named - set(long[:3]), key=lambda l: -m2.cls[l])
    assert "max_long is 2" in problems(long[:3], 3 * 1008, rest, m2)
    m3 = M.model_of(M.caps(0, 3 * 1008 + M.SLACK - 1))
    assert "over long_bytes" in problems(long[:3], 3 * 1008, rest, m3)
    rest1 = sorted(m3.named - set(long[:1]), key=lambda l: -m3.cls[l])
    assert "the header says 2" in problems(long[:1], 1008, rest1, m3)
    # every long list fits, and one stayed a lane
    assert "the header says 5" in problems(long[1:], nbytes - 1008, sorted(short + long[:1], key=lambda l: -m.cls[l]))


def test_workspace_layouts_and_growth_under_asan_ubsan(tmp_path):
    """The planned and the routed workspace layout against their formulas written out, and
    the grow / refuse decision of a device call's workspace (tests/cpp/call_workspace_check.cpp)."""
    exe = tmp_path / "call_workspace_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "call_workspace_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    # n x with_list x (the planned layout + m x flat_bytes routed ones); capacity x need x spare x capturing
    assert "call_workspace ok: %d layouts, %d growth decisions" % (7 * 2 * (1 + 3 * 3), 4 * 4 * 3 * 2) in r.stdout


def _room_ok(given, length, long_bytes):
    """parts_route.hpp room_ok restated in Python integers."""
    r = (length + 15) // 16 * 16
    ok = given + r + M.SLACK <= long_bytes
    return ok, (given + r if ok else 0)


def test_claim_arithmetic_under_asan_ubsan(tmp_path):
    top = (1 << 64) - 1
    triples = []
    for long_bytes in (0, 63, 64, 79, 80, 81, 1008 + 64, 3 * 1008 + 64, 3 * 1008 + 63, 32 << 20, 1 << 48, top):
        for given in (0, 16, 1008, 2016, long_bytes - 64 if long_bytes >= 64 else 0, top - 15, top):
            for length in (0, 1, 15, 16, 17, 1000, 1008, 1009, top - 16, top - 15, top - 14, top):
                triples.append((given, length, long_bytes))
    triples = sorted(set(triples))
    assert (2016, 1000, 3 * 1008 + 64) in triples and (2016, 1000, 3 * 1008 + 63) in triples    # exact fit, one byte over
    exe = tmp_path / "parts_route_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "parts_route_check.cpp")], check=True)
    args = [str(v) for t in triples for v in t]
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert re.search(r"parts_route ok: %d edges, \d+ replays" % len(triples), r.stdout)
    got = {}
    for line in r.stdout.splitlines():
        if line.startswith("E "):
            g, n, b, ok, nxt = map(int, line.split()[1:])
            got[(g, n, b)] = (bool(ok), nxt)
    assert got == {t: _room_ok(*t) for t in triples}
    assert got[(2016, 1000, 3 * 1008 + 64)] == (True, 3024) and got[(2016, 1000, 3 * 1008 + 63)] == (False, 0)
