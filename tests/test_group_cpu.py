"""The probe, the layout and the numbering of msha_group_digests_device
(mirbft_amd/csrc/group.hpp) under AddressSanitizer + UBSan, as a stand-alone program with
its own main (tests/cpp/group_check.cpp) over every case the GPU test launches
(tests/group_matrix.py), the insert in three slot orders, its results compared with the
numpy oracle; the cases proven to cover what they claim; and the oracle shown to follow
the header and to reject wrong results. Host code only: nothing is loaded into Python."""
import os
import subprocess

import numpy as np

import group_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cases_cover_what_they_claim():
    T, S = M.tile(), M.scan_slots()
    assert T % 64 == 0 and S % T == 0 and S > 8 * T + 1
    assert M.sizes() == [1, 2, 63, 64, 65, 255, 256, 257, 8 * T - 1, 8 * T + 1, S - 1, S, S + 1, 2 * S + 1]
    for n in (1, 2, 257, 2 * S + 1):
        p = M.patterns(n)
        assert set(p) == {"distinct", "one", "two", "mirrored", "last_leader", "random"}
        assert all(v.size == n for v in p.values())
        assert np.unique(p["distinct"]).size == n and np.unique(p["one"]).size == 1
        assert np.unique(p["two"]).size == min(n, 2)
        m = p["mirrored"]
        assert (m == m[::-1]).all() and np.unique(m).size == (n + 1) // 2
        want = M.oracle(M.base_rows(m).reshape(-1), None, n)
        assert (want[3][:want[5][1]] < (n + 1) // 2).all()             # every leader in the first half
        last = M.oracle(M.base_rows(p["last_leader"]).reshape(-1), None, 4)
        assert last[5][1] == min(n, 2) and last[3][last[5][1] - 1] == n - 1
        assert p["random"].max() < max(1, n // 10)
    # one byte apart, all 32 positions: two groups where one would be wrong
    assert sorted(c.flips[0][1] for c in M.byte_cases()) == list(range(32))
    for c in M.byte_cases():
        d = c.digests().reshape(65, 32)
        assert (d[40] != d[3]).sum() == 1 and c.flips[0][0] == 40
        want = M.case_oracle(c)
        assert want[5][:2] == (65, 65) and want[0][40] == 40 and want[1][40] != want[1][3]
    three, bit31, zero, null = M.scope_cases()
    assert np.unique(three.val).size == 1 and M.case_oracle(three)[5][1] == 3
    assert set(bit31.scope.tolist()) == {0, 1 << 31} and M.case_oracle(bit31)[5][1] == 2
    assert null.scope is None and not zero.scope.any() and (zero.val == null.val).all()
    assert M.problems(M.case_oracle(zero), M.case_oracle(null)) == []
    caps = M.cap_cases()
    g = M.case_oracle(caps[0])[5][1]
    assert g == M.CAP_GROUPS and [c.group_cap for c in caps] == [0, 1, g - 1, g, g + 1]
    probes = M.probe_cases()
    assert [c.force_home() for c in probes] == [0, 0, M.capacity(300) - 2, M.capacity(300) - 2]
    assert all(c.n == 300 for c in probes) and M.capacity(300) == 1024
    assert M.case_oracle(probes[0])[5][1] == 300 and 1 < M.case_oracle(probes[1])[5][1] <= 40
    assert [M.capacity(n) for n in (1, 32, 33, 64, 65, 2**30)] == [64, 64, 128, 128, 256, 2**31]
    names = [c.name for c in M.all_cases()]
    assert len(set(names)) == len(names)


def test_oracle_follows_the_header():
    """A hand-worked example: rows B A B C A A under one scope, then under two."""
    rows = M.base_rows([7, 5, 7, 9, 5, 5]).reshape(-1)
    first, group, members, gf, gc, res = M.oracle(rows, None, 4)
    assert first.tolist() == [0, 1, 0, 3, 1, 1] and group.tolist() == [0, 1, 0, 2, 1, 1]
    assert members.tolist() == [2, 3, 2, 1, 3, 3]
    assert gf.tolist() == [0, 1, 3, M.SENTINEL] and gc.tolist() == [2, 3, 1, M.SENTINEL]
    assert res == (6, 3, 3, 3, 1)
    # group_cap cuts the list, not the count; a tie for the largest goes to the smaller id
    first, group, members, gf, gc, res = M.oracle(M.base_rows([7, 5, 7, 5]).reshape(-1), None, 1)
    assert res == (4, 2, 1, 2, 0) and gf.tolist() == [0] and gc.tolist() == [2]
    # the scope is part of the key
    scope = np.array([0, 0, 1, 0, 0, 1], dtype=np.uint32)
    first, group, members, gf, gc, res = M.oracle(rows, scope, 8)
    assert first.tolist() == [0, 1, 2, 3, 1, 5] and group.tolist() == [0, 1, 2, 3, 1, 4]
    assert res == (6, 5, 5, 2, 1) and gf[:5].tolist() == [0, 1, 2, 3, 5] and gc[:5].tolist() == [1, 2, 1, 1, 1]
    assert (gf[5:] == M.SENTINEL).all()


def test_problems_reject_wrong_results():
    c = M.cap_cases()[2]                            # group_cap = groups - 1
    want = M.case_oracle(c)
    assert M.problems(want, want) == []
    first, group, members, gf, gc, res = want
    g2 = group.copy()
    a, b = group == 3, group == 4
    g2[a], g2[b] = 4, 3                             # a swapped pair of group ids
    assert any("group differs" in p for p in M.problems(want, (first, g2, members, gf, gc, res)))
    c2 = gc.copy()
    c2[5] += 1                                      # a wrong count
    assert any("group_count differs" in p for p in M.problems(want, (first, group, members, gf, c2, res)))
    m2 = members.copy()
    m2[17] -= 1
    assert any("members differs" in p for p in M.problems(want, (first, group, m2, gf, gc, res)))
    short = M.oracle(c.digests(), None, c.group_cap + 3)
    over = short[3].copy()
    assert over[res[2] + 1] == M.SENTINEL
    over[res[2] + 1] = 0                            # a written entry past listed
    assert any("group_first differs" in p for p in M.problems(short, short[:3] + (over,) + short[4:]))
    assert any("result" in p for p in M.problems(want, (first, group, members, gf, gc, res[:4] + (res[4] + 1,))))
    assert M.problems(want, (first, group, None, gf, gc, res)) == []     # a call without d_members


def test_probe_and_numbering_under_asan_ubsan(tmp_path):
    cases = M.all_cases()
    path, results = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    M.write_cases(path, cases)
    exe = tmp_path / "group_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "group_check.cpp")], check=True)
    r = subprocess.run([str(exe), path, results], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "layout checked" in r.stdout and "group ok: %d cases" % len(cases) in r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("case ")]
    got = M.read_results(results, cases)
    for k, (c, g) in enumerate(zip(cases, got)):
        want = M.case_oracle(c)
        assert M.problems(want, g) == [], c.name
        assert lines[k] == "case %d: n %d groups %d listed %d max_count %d max_group %d" % ((k,) + want[5]), c.name
