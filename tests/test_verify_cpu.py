"""The layout and the walk of msha_verify_digests_device (mirbft_amd/csrc/verify.hpp)
under AddressSanitizer + UBSan, as a stand-alone program with its own main
(tests/cpp/verify_check.cpp) over every case the GPU test launches
(tests/verify_matrix.py), its results compared with the numpy oracle; the cases proven
to cover what they claim; and the oracle shown to follow the header and to reject wrong
results. Host code only: nothing is loaded into Python."""
import os
import subprocess

import numpy as np

import verify_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cases_cover_what_they_claim():
    W = M.scan_words()
    assert W >= 64 and {1, 63, 64, 65, 255, 256, 257, 4095, 4097, 64 * W - 1, 64 * W, 64 * W + 1,
                        2 * 64 * W + 1} <= set(M.sizes(W))
    big = M.patterns(2 * 64 * W + 1, W)
    assert set(big) == {"none", "all", "first", "last", "word_edge", "chunk_edge", "random"}
    assert big["chunk_edge"] == [64 * W - 1, 64 * W] and big["word_edge"] == [63, 64]
    assert len(big["random"]) == (2 * 64 * W + 1) // 100 and big["last"] == [2 * 64 * W]
    assert set(M.patterns(1, W)) == {"none", "all", "first", "last", "random"}
    # one byte of the expected digest each, all 32 positions
    assert sorted(c.flips[0][2] for c in M.byte_cases()) == list(range(32))
    for c in M.byte_cases():
        got, exp = c.arrays()
        assert (got.reshape(65, 32) != exp.reshape(65, 32)).sum() == 1 and M.case_oracle(c)[1] == (65, 1, 40, 1, 0)
    caps = M.list_cases(W)
    assert [c.list_cap for c in caps[:5]] == [0, 1, 39, 40, 41] and all(len(c.flips) == 40 for c in caps[:5])
    mid, edge = caps[5], caps[6]
    chunk = 64 * W
    for c in (mid, edge):
        assert M.case_oracle(c)[1][1] > c.list_cap          # the list is cut short in both
    in_first = sum(1 for _, s, _ in edge.flips if s < chunk)
    assert edge.list_cap == in_first and in_first < mid.list_cap < sum(1 for _, s, _ in mid.flips if s < 2 * chunk)
    rep, perm, oob = M.index_cases()
    assert rep.n == 257 and rep.n_expected == 4 and set(rep.idx.tolist()) == {0, 1, 2, 3}
    assert sorted(perm.idx.tolist()) == list(range(4097))
    assert (oob.idx == 200).sum() == 2 and (oob.idx == 0xFFFFFFFF).sum() == 1 and M.case_oracle(oob)[1][4] == 3


def test_oracle_follows_the_header():
    got = M.base_rows(np.arange(70)).copy()
    exp = got.copy()
    got[3, 31] ^= 1
    got[63, 0] ^= 0x80
    got[64, 17] ^= 1
    mask, res, lst = M.oracle(got.reshape(-1), exp.reshape(-1), None, 70, 2)
    assert mask.tolist() == [(1 << 3) | (1 << 63), 1] and res == (70, 3, 3, 2, 0)
    assert lst.tolist() == [3, 63]
    mask, res, lst = M.oracle(exp.reshape(-1), exp.reshape(-1), None, 70, 3)
    assert not mask.any() and res == (70, 0, 70, 0, 0) and lst.tolist() == [M.LIST_SENTINEL] * 3
    # indices: a repeat, and two out of range which differ whatever the rows hold
    idx = np.array([1, 1, 2, 0xFFFFFFFF], dtype=np.uint32)
    g = M.base_rows([1, 1, 2, 0]).reshape(-1)
    mask, res, lst = M.oracle(g, M.base_rows(np.arange(2)).reshape(-1), idx, 2, 4)
    assert mask.tolist() == [0b1100] and res == (4, 2, 2, 2, 2) and lst.tolist()[:2] == [2, 3]


def test_problems_reject_wrong_results():
    c = M.list_cases(M.scan_words())[3]
    want = M.case_oracle(c)
    assert M.problems(want, want) == []
    mask, res, lst = want
    m = mask.copy()
    m[-1] |= np.uint64(1) << np.uint64(63)                    # a bit past n in the last word
    assert any("mask differs" in p for p in M.problems(want, (m, res, lst)))
    l2 = lst.copy()
    l2[0], l2[1] = lst[1], lst[0]                             # the list out of order
    assert any("list differs" in p for p in M.problems(want, (mask, res, l2)))
    assert any("result" in p for p in M.problems(want, (mask, res[:2] + (res[2] + 1,) + res[3:], lst)))


def test_walk_under_asan_ubsan(tmp_path):
    cases = M.all_cases(M.scan_words())
    path, results = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    M.write_cases(path, cases)
    exe = tmp_path / "verify_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "verify_check.cpp")], check=True)
    r = subprocess.run([str(exe), path, results], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "verify ok: %d cases" % len(cases) in r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("case ")]
    got = M.read_results(results, cases)
    for k, (c, g) in enumerate(zip(cases, got)):
        want = M.case_oracle(c)
        assert M.problems(want, g) == [], c.name
        assert lines[k] == "case %d: n %d bad %d first_bad %d listed %d bad_index %d" % ((k,) + want[1]), c.name
