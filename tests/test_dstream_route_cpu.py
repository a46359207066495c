"""The route model of msha_dstreams_write_routed_device (tests/dstream_route_matrix.py):
each builder proven, by set equality, to reach what it claims; every case that is not a
caps case shown to fit both caps under the model alone, so the GPU tests may demand that
routed equals long exactly; check_route() shown to reject wrong routes; and the
host-checkable decisions of mirbft_amd/csrc/stream_chain.hpp -- the barrier schedule of
k_absorb_chain8 first of all -- under AddressSanitizer + UBSan as a stand-alone program
with its own main (tests/cpp/stream_chain_check.cpp). Host code only: nothing is loaded
into Python."""
import os
import re
import subprocess

import numpy as np

import dstream_matrix
import dstream_route_matrix as M
from mirbft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mirbft_amd", "csrc")


def _const(header, name):
    text = open(os.path.join(CSRC, header)).read()
    return int(re.search(r"constexpr \w+ %s = (\d+);" % name, text).group(1))


def _counts(begin):
    return [int(b) - int(a) for a, b in zip(begin, begin[1:])]


def _pre_leaves_the_tails(case):
    m = dstream_matrix.Model(case.n)
    m.write(case.pre)
    assert m.length == list(case.tails) and all(t < 64 for t in case.tails)


def _fits(case):
    r = M.model_of(case)
    assert r.all_fit and r.count == len(r.long)
    assert len(r.long) <= case.max_long <= 16 * 8             # 16 x CUs of the smallest part one could meet
    assert sum(M.round16(r.total[x]) for x in r.long) + M.SLACK <= case.long_bytes
    return r


def test_constants_are_the_sources():
    assert M.SLACK == L.MSHA_DEVICE_ARENA_SLACK
    assert L.MSHA_DSTREAMS_ROUTE_LONG_BLOCKS_DEFAULT == 64
    header = open(L.HEADER_PATH).read()
    assert "#define MSHA_DSTREAMS_ROUTE_LONG_BLOCKS_DEFAULT 64u" in header
    assert _const("kernels.hpp", "kChain8MsgsPerWg") == 16
    assert _const("stream_chain.hpp", "kPairMinBlocks") == _const("kernels.hip", "kC2PairMinBlocks") == 64
    assert _const("stream_chain.hpp", "kProducers") == _const("kernels.hip", "kC8Producers") == 2


def test_threshold_edge_covers_what_it_claims():
    for lb in (2, 3, 4):
        case, combos = M.threshold_edge(lb)
        _pre_leaves_the_tails(case)
        r = _fits(case)
        assert {t for t, _, _ in combos} == {0, 1, 55, 56, 63} and len(combos) == 30
        assert {(lx, d) for _, lx, d in combos} == {(x, d) for x in (lb, lb + 1) for d in (-1, 0, 1)}
        sums = [sum(int(x) for x in case.batch[2][int(a):int(b)]) for a, b in zip(case.batch[3], case.batch[3][1:])]
        assert [case.tails[i] + sums[i] for i in range(30)] == [64 * lx + d for _, lx, d in combos]
        assert r.long == {i for i, (_, lx, d) in enumerate(combos) if not (lx == lb and d == -1)}
        assert {r.whole[i] for i in range(30)} == {lb - 1, lb, lb + 1} and len(r.long) == 25


def test_new_tail_edges_cover_what_they_claim():
    case, combos = M.new_tail_edges()
    _pre_leaves_the_tails(case)
    r = _fits(case)
    assert r.long == set(range(len(combos))) and len(combos) == 18
    assert {r.total[i] % 64 for i in r.long} == {0, 1, 15, 16, 17, 63}
    assert {(case.tails[i], r.total[i] % 64) for i in r.long} == {(t, k) for t in (0, 17, 63) for k in M.NEW_TAILS}
    assert {r.whole[i] for i in r.long} == {2, 3}


def test_gather_paths_cover_what_they_claim():
    case, (three, many, short) = M.gather_paths()
    _pre_leaves_the_tails(case)
    r = _fits(case)
    counts = _counts(case.batch[3])
    assert counts == [3, 300, 2] and r.long == {three, many} and short not in r.long
    off, ln, begin = case.batch[1], case.batch[2], case.batch[3]
    j = int(begin[three]) + 1
    assert int(ln[j]) == 2000 and int(off[j]) % 2 == 1
    lens = ln[int(begin[many]): int(begin[many + 1])]
    assert int(lens.max()) <= 40 and int((lens == 0).sum()) >= 18
    step, large, wave = _const("parts_concat.hpp", "kStepParts"), _const("parts_concat.hpp", "kLargePart"), \
        _const("parts_plan.hpp", "kWaveSumParts")
    # + 1: the stream's buffered bytes are the copy's part 0
    assert counts[three] < wave <= counts[many] and counts[many] + 1 > step and 2000 >= large
    assert case.tails[three] and case.tails[many]


def test_slot_cases_cover_what_they_claim():
    for k in (1, 8, 9, 16, 17):
        for permute in (False, True):
            case, routed = M.slots(k, permute=permute)
            _pre_leaves_the_tails(case)
            r = _fits(case)
            assert r.long == set(routed) and len(routed) == k
            assert {r.whole[x] for x in routed} == set(range(2, 2 + min(k, 4)))
            assert (case.rows is None) != permute
            if permute:
                assert len(set(case.rows.tolist())) == case.rows.size and int(case.rows.max()) < case.n
                assert case.rows.tolist() != sorted(case.rows.tolist())
            assert 0 in _counts(case.batch[3])                      # a zero-part row among them
    case, routed = M.slots(4, big=True)
    r = _fits(case)
    assert [r.whole[x] for x in routed] == [65, 3, 4, 5]
    # 65 blocks enters the pair path (>= 64) with an odd count; the others of the workgroup end long before
    assert 65 >= _const("stream_chain.hpp", "kPairMinBlocks") and 65 % 2 == 1


def test_caps_cases():
    r16 = M.round16(M.CAP_TOTAL)
    assert r16 == 1008 and M.CAP_TOTAL // 64 == 15
    for max_long, long_bytes, want, fit in ((1, M.LONG_BYTES, 1, False), (2, M.LONG_BYTES, 2, False),
                                            (5, M.LONG_BYTES, 5, True), (64, 3 * r16 + M.SLACK, 3, False),
                                            (64, 3 * r16 + M.SLACK - 1, 2, False), (64, 5 * r16 + M.SLACK, 5, True),
                                            (64, 5 * r16 + M.SLACK - 1, 4, False), (4, 2 * r16 + M.SLACK + 15, 2, False)):
        case = M.caps(max_long, long_bytes)
        _pre_leaves_the_tails(case)
        r = M.model_of(case)
        assert r.long == {0, 2, 3, 5, 7} and {r.total[x] for x in r.long} == {M.CAP_TOTAL}
        assert (r.count, r.all_fit) == (want, fit), (max_long, long_bytes)


def test_error_case_covers_what_it_claims():
    case, (bad_stream, bad_range, _) = M.errors()
    _pre_leaves_the_tails(case)
    r = _fits(case)
    begin, ln = case.batch[3], case.batch[2]
    assert r.invalid_stream == [bad_stream] and r.invalid_range == [bad_range]
    assert int(case.rows[bad_stream]) >= case.n and int(begin[bad_range + 1]) < int(begin[bad_range])
    between = int(ln[int(begin[bad_range + 1]): int(begin[bad_range])].sum())
    assert between // 64 >= case.long_blocks                         # long by the parts between its bounds
    assert int(ln[int(begin[bad_stream]): int(begin[bad_stream + 1])].sum()) // 64 >= case.long_blocks
    assert len(r.long) >= 2 and bad_stream not in r.long and bad_range not in r.long
    assert set(range(6)) - r.long - {bad_stream, bad_range}          # and a short, valid row


def test_no_long_and_rounds_cases():
    case = M.no_long()
    _pre_leaves_the_tails(case)
    r = _fits(case)
    assert r.long == set() and max(r.whole.values()) == case.long_blocks - 1 and len(r.whole) == 70
    case = M.rounds_case()
    _pre_leaves_the_tails(case)
    for tails in ([0] * 6, [63] * 6, case.tails):                    # whatever the rounds before left
        r = M.model_of(case, tails)
        assert r.long == {0, 1, 3, 5} and r.all_fit


def test_check_route_rejects_wrong_routes():
    case, routed = M.slots(8)
    r = M.model_of(case)
    nbytes = sum(M.round16(r.total[x]) for x in routed)
    assert M.check_route(routed, nbytes, r) == []
    assert M.check_route(routed[::-1], nbytes, r) == []

    def problems(ids, b, route=r):
        return " | ".join(M.check_route(ids, b, route))

    short = sorted(set(r.whole) - r.long)[0]
    assert "is routed and is not long" in problems(routed + [short], nbytes)
    assert "is not long" in problems(routed[1:], nbytes - M.round16(r.total[routed[0]]))
    assert "routed twice" in problems(routed + routed[:1], nbytes)
    assert "routed_bytes" in problems(routed, nbytes + 16)
    r2 = M.model_of(M.caps(2, M.LONG_BYTES))
    assert M.check_route([0, 5], 2 * 1008, r2) == [] and M.check_route([7, 3], 2 * 1008, r2) == []
    assert "the header says 2" in problems([0, 2, 3], 3 * 1008, r2)
    assert "the header says 2" in problems([0], 1008, r2)


def test_decisions_under_asan_ubsan(tmp_path):
    exe = tmp_path / "stream_chain_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "stream_chain_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    m = re.search(r"stream_chain ok: (\d+) barrier schedules, (\d+) decisions, (\d+) tails", r.stdout)
    assert m and int(m.group(1)) == 2 * 201 and int(m.group(2)) > 60000 and int(m.group(3)) == 320


def test_model_matches_numpy_on_whole_blocks():
    """The model's `whole` restated once more from the bytes: what a hashlib-fed stream
    would have compressed."""
    case, _ = M.threshold_edge()
    r = M.model_of(case)
    arena, off, ln, begin = case.batch
    for row in range(begin.size - 1):
        data = b"".join(arena[int(off[j]): int(off[j]) + int(ln[j])].tobytes()
                        for j in range(int(begin[row]), int(begin[row + 1])))
        assert (case.tails[row] + len(data)) // 64 == r.whole[row]
    assert isinstance(case.batch[3], np.ndarray)
